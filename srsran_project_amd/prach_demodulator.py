"""Host-side mirror of srsRAN's PRACH OFDM demodulator over the MI355X C-ABI (include/srsran_amd/prach_demodulator.h).

Reference interface:
  ofdm_prach_demodulator.h:79    demodulate(prach_buffer& buffer, span<const cf_t> input, const configuration& config)

One call demodulates every port, time-domain and frequency-domain occasion of any number of windows; the output
blocks are the occasions PrachDetector.detect_batch reads (detector_offsets()).
"""
import ctypes
from dataclasses import dataclass
from typing import List

import numpy as np

from . import _lib

MAX_TD_OCCASIONS = 7
MAX_FD_OCCASIONS = 8


class _Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "numerology", "subframe_slot_index", "format", "nof_td_occasions", "nof_fd_occasions", "start_symbol",
        "rb_offset", "nof_prb_ul_grid", "nof_ports")]


class _Geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "ra_scs", "L_ra", "dft_size", "nof_symbols", "sub_dft_size", "nof_sub_dfts")] + [
        ("window_samples", ctypes.c_uint64), ("min_input_samples", ctypes.c_uint64), ("nof_elements", ctypes.c_uint64),
        ("sample_offset", ctypes.c_uint32 * MAX_TD_OCCASIONS), ("cp_samples", ctypes.c_uint32 * MAX_TD_OCCASIONS),
        ("k_start", ctypes.c_uint32 * MAX_FD_OCCASIONS)]


_declared = False


def _L():
    global _declared
    lib = _lib.lib()
    if not _declared:
        c, P, U64P = ctypes, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
        for name, res, args in [
            ("srs_amd_prach_demodulator_create", c.c_int, [c.POINTER(P), c.c_uint32, c.c_int]),
            ("srs_amd_prach_demodulator_destroy", None, [P]),
            ("srs_amd_prach_demod_get_geometry", c.c_int, [c.c_uint32, c.POINTER(_Config), c.POINTER(_Geometry)]),
            ("srs_amd_prach_demod_get_detector_offsets", c.c_int, [c.c_uint32, c.POINTER(_Config), c.c_uint64, U64P]),
            ("srs_amd_prach_demodulate", c.c_int, [P, c.POINTER(_Config), P, c.c_uint64, c.c_uint64, P]),
            ("srs_amd_prach_demodulate_batch", c.c_int,
             [P, c.POINTER(_Config), c.c_uint32, P, U64P, U64P, U64P, P, U64P, P]),
        ]:
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _declared = True
    return lib


@dataclass
class PrachDemodConfiguration:
    """ofdm_prach_demodulator::configuration without `port`: all nof_ports ports are demodulated in one call."""
    format: int
    numerology: int = 0
    subframe_slot_index: int = 0
    nof_td_occasions: int = 1
    nof_fd_occasions: int = 1
    start_symbol: int = 0
    rb_offset: int = 0
    nof_prb_ul_grid: int = 0
    nof_ports: int = 1

    def _c(self):
        return _Config(int(self.numerology), int(self.subframe_slot_index), int(self.format),
                       int(self.nof_td_occasions), int(self.nof_fd_occasions), int(self.start_symbol),
                       int(self.rb_offset), int(self.nof_prb_ul_grid), int(self.nof_ports))


@dataclass
class PrachDemodGeometry:
    """What the demodulator derives from a sampling rate and a configuration."""
    ra_scs: int
    L_ra: int
    dft_size: int
    nof_symbols: int
    sub_dft_size: int
    nof_sub_dfts: int
    window_samples: int
    min_input_samples: int
    nof_elements: int
    sample_offset: List[int]  # per time-domain occasion
    cp_samples: List[int]     # per time-domain occasion
    k_start: List[int]        # per frequency-domain occasion


def prach_demod_geometry(srate_hz, config):
    """Validates `config` at `srate_hz` as the demodulate calls do (ValueError) and returns its geometry; needs no
    device."""
    g, c = _Geometry(), config._c()
    _lib.check(_L().srs_amd_prach_demod_get_geometry(int(srate_hz), ctypes.byref(c), ctypes.byref(g)),
               "PRACH demodulator geometry")
    ntd, nfd = int(config.nof_td_occasions), int(config.nof_fd_occasions)
    return PrachDemodGeometry(int(g.ra_scs), int(g.L_ra), int(g.dft_size), int(g.nof_symbols), int(g.sub_dft_size),
                              int(g.nof_sub_dfts), int(g.window_samples), int(g.min_input_samples),
                              int(g.nof_elements), list(g.sample_offset)[:ntd], list(g.cp_samples)[:ntd],
                              list(g.k_start)[:nfd])


def prach_detector_offsets(srate_hz, config, out_offset=0):
    """Element offsets of the window's occasions, [td x nof_fd + fd]: each block is one occasion of
    PrachDetector.detect_batch with nof_rx_ports = config.nof_ports."""
    n = int(config.nof_td_occasions) * int(config.nof_fd_occasions)
    offs, c = (ctypes.c_uint64 * max(n, 1))(), config._c()
    _lib.check(_L().srs_amd_prach_demod_get_detector_offsets(int(srate_hz), ctypes.byref(c), int(out_offset), offs),
               "PRACH demodulator offsets")
    return [int(o) for o in offs[:n]]


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


class PrachDemodBatch:
    """The configurations and buffer layout of a batch in the C layout, validated once (ValueError): for a static
    cell configuration, so that a call does no per-window work in Python."""

    def __init__(self, srate_hz, configs, sample_offsets, nof_samples, port_strides=None, out_offsets=None):
        self.n = len(configs)
        geos = [prach_demod_geometry(srate_hz, c) for c in configs]
        if port_strides is None:
            port_strides = nof_samples
        if out_offsets is None:
            sizes = [g.nof_elements for g in geos]
            out_offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if sizes else []
        if not (len(sample_offsets) == len(nof_samples) == len(port_strides) == len(out_offsets) == self.n):
            raise ValueError("one sample offset, sample count, port stride and output offset per window")
        if any(int(v) < 0 for v in list(sample_offsets) + list(out_offsets)):
            raise ValueError("negative offset")
        self.samples_needed = max([int(o) + (int(c.nof_ports) - 1) * int(st) + int(m) for c, o, m, st in
                                   zip(configs, sample_offsets, nof_samples, port_strides)], default=0)
        self.elements_needed = max([int(o) + g.nof_elements for o, g in zip(out_offsets, geos)], default=0)
        self.out_offsets = [int(o) for o in out_offsets]
        self.cfgs = (_Config * max(self.n, 1))(*[c._c() for c in configs])
        self.s_off, self.strides, self.nof = _u64(sample_offsets), _u64(port_strides), _u64(nof_samples)
        self.o_off = _u64(out_offsets)


class PrachDemodulator:
    """``ofdm_prach_demodulator`` on the GPU, any number of windows per call."""

    def __init__(self, srate_hz, device=-1):
        self._lib = _L()
        self.srate_hz = int(srate_hz)
        h = ctypes.c_void_p()
        _lib.check(self._lib.srs_amd_prach_demodulator_create(ctypes.byref(h), self.srate_hz, int(device)),
                   "PRACH demodulator create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srs_amd_prach_demodulator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def geometry(self, config):
        return prach_demod_geometry(self.srate_hz, config)

    def detector_offsets(self, configs, out_offsets=None):
        """The detect_batch offsets of every occasion of every window, in window order, for outputs packed back to
        back (default) or at `out_offsets`."""
        if out_offsets is None:
            out_offsets = self.packed_offsets(configs)
        return [o for c, base in zip(configs, out_offsets) for o in prach_detector_offsets(self.srate_hz, c, base)]

    def packed_offsets(self, configs):
        sizes = [self.geometry(c).nof_elements for c in configs]
        return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if sizes else []

    def demodulate(self, samples, config, nof_samples=None):
        """Host form, one window.  samples: complex64 [ports, port_stride] (or one row for one port), of which the
        first nof_samples of every row are valid (default: all).  Returns uint16 [td, fd, ports, symbols, L_ra, 2]
        cbf16 bit patterns (re, im)."""
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(samples)), np.complex64)
        g = self.geometry(config)
        if x.shape[0] != int(config.nof_ports):
            raise ValueError("samples hold %d ports, the configuration %d" % (x.shape[0], config.nof_ports))
        out = np.empty((int(config.nof_td_occasions), int(config.nof_fd_occasions), int(config.nof_ports),
                        g.nof_symbols, g.L_ra, 2), np.uint16)
        c = config._c()
        n = x.shape[1] if nof_samples is None else int(nof_samples)
        if not 0 <= n <= x.shape[1]:
            raise ValueError("nof_samples exceeds the %d samples of a row" % x.shape[1])
        _lib.check(self._lib.srs_amd_prach_demodulate(self._h, ctypes.byref(c), x.ctypes.data, n, x.shape[1],
                                                      out.ctypes.data), "PRACH demodulate")
        return out

    def demodulate_batch(self, samples, configs, sample_offsets=None, nof_samples=None, port_strides=None, out=None,
                         out_offsets=None, stream=None):
        """Device form, asynchronous.  samples: one contiguous complex64 (or float32 pairs) device tensor; window i's
        port p starts sample_offsets[i] + p x port_strides[i] complex samples into it and holds nof_samples[i]
        (port_strides default: nof_samples).  out: device tensor of cbf16 words (int32 / uint32, or 16-bit pairs),
        window i at out_offsets[i] elements (default: packed back to back; allocated when None).  configs: a list of
        PrachDemodConfiguration with those arrays, or a PrachDemodBatch prepared once.  Returns out."""
        import torch

        if not samples.is_cuda or not samples.is_contiguous():
            raise ValueError("samples must be a contiguous device tensor")
        batch = configs if isinstance(configs, PrachDemodBatch) else PrachDemodBatch(
            self.srate_hz, configs, sample_offsets, nof_samples, port_strides, out_offsets)
        have = samples.numel() * samples.element_size() // 8
        if batch.samples_needed > have:
            raise ValueError("a window reaches beyond the %d samples of the buffer" % have)
        need = batch.elements_needed
        if out is None:
            out = torch.empty(need, dtype=torch.int32, device=samples.device)
        elif (not out.is_cuda or not out.is_contiguous() or out.device != samples.device
              or out.numel() * out.element_size() // 4 < need):
            raise ValueError("out must be a contiguous device tensor of at least %d cbf16 elements" % need)
        if stream is None:
            stream = torch.cuda.current_stream(samples.device)
        _lib.check(self._lib.srs_amd_prach_demodulate_batch(
            self._h, batch.cfgs, batch.n, samples.data_ptr(), batch.s_off, batch.strides, batch.nof,
            out.data_ptr(), batch.o_off, ctypes.c_void_p(stream.cuda_stream)), "PRACH demodulate batch")
        return out
