"""Host-side mirror of srsRAN's PRACH detector over the MI355X C-ABI (include/srsran_amd/prach.h).

Reference interfaces:
  prach_detector.h:79            detect(const prach_buffer& input, const configuration& config)
  prach_detection_result.h:30    prach_detection_result

The detection threshold and the window margin are part of the configuration: the reference reads them from a table
tuned for its own detector (detail::get_threshold_and_margin); here the integrator supplies them.
"""
import ctypes
import enum
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import _lib

MAX_PREAMBLES = 64


class PrachFormat(enum.IntEnum):
    """srs_amd_prach_format (the reference's prach_format_type)."""
    ZERO = 0
    ONE = 1
    TWO = 2
    THREE = 3
    A1 = 4
    A2 = 5
    A3 = 6
    B1 = 7
    B4 = 8
    C0 = 9
    C2 = 10
    A1_B1 = 11
    A2_B2 = 12
    A3_B3 = 13


class PrachSubcarrierSpacing(enum.IntEnum):
    """srs_amd_prach_scs (the reference's prach_subcarrier_spacing)."""
    KHZ15 = 0
    KHZ30 = 1
    KHZ60 = 2
    KHZ120 = 3
    KHZ1_25 = 4
    KHZ5 = 5


class _Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "format", "ra_scs", "root_sequence_index", "zero_correlation_zone", "restricted_set", "start_preamble_index",
        "nof_preamble_indices", "nof_rx_ports", "combine_symbols", "idft_size")] + [
        ("threshold", ctypes.c_float), ("win_margin", ctypes.c_uint32)]


class _Geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "L_ra", "N_cs", "nof_shifts", "nof_sequences", "win_width", "max_delay_samples", "nof_symbols",
        "idft_size")] + [("nof_elements", ctypes.c_uint64)]


class _Preamble(ctypes.Structure):
    _fields_ = [("preamble_index", ctypes.c_uint32), ("delay_samples", ctypes.c_int32),
                ("time_advance_s", ctypes.c_double), ("detection_metric", ctypes.c_float),
                ("preamble_power_db", ctypes.c_float)]


class _Window(ctypes.Structure):
    _fields_ = [("peak_over_threshold", ctypes.c_float), ("delay_samples", ctypes.c_int32)]


class _Result(ctypes.Structure):
    _fields_ = [("rssi_db", ctypes.c_float), ("nof_detected", ctypes.c_uint32),
                ("time_resolution_s", ctypes.c_double), ("time_advance_max_s", ctypes.c_double),
                ("preambles", _Preamble * MAX_PREAMBLES), ("windows", _Window * MAX_PREAMBLES)]


RESULT_BYTES = ctypes.sizeof(_Result)

_declared = False


def _L():
    global _declared
    lib = _lib.lib()
    if not _declared:
        c, P = ctypes, ctypes.c_void_p
        for name, res, args in [
            ("srs_amd_prach_detector_create", c.c_int, [c.POINTER(P), c.c_int]),
            ("srs_amd_prach_detector_destroy", None, [P]),
            ("srs_amd_prach_get_geometry", c.c_int, [c.POINTER(_Config), c.POINTER(_Geometry)]),
            ("srs_amd_prach_physical_root", c.c_uint32, [c.c_uint32, c.c_uint32]),
            ("srs_amd_prach_detect", c.c_int, [P, c.POINTER(_Config), P, c.POINTER(_Result)]),
            ("srs_amd_prach_detect_batch", c.c_int,
             [P, c.POINTER(_Config), c.c_uint32, P, c.POINTER(c.c_uint64), P, P]),
        ]:
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _declared = True
    return lib


@dataclass
class PrachConfiguration:
    """prach_detector::configuration, plus combine_symbols / idft_size (fixed at construction in the reference) and
    the threshold and window margin (looked up in the reference)."""
    format: int
    ra_scs: int
    root_sequence_index: int
    zero_correlation_zone: int
    threshold: float
    win_margin: int
    nof_rx_ports: int = 1
    start_preamble_index: int = 0
    nof_preamble_indices: int = 64
    combine_symbols: bool = True
    idft_size: int = 0
    restricted_set: int = 0

    def _c(self):
        return _Config(int(self.format), int(self.ra_scs), int(self.root_sequence_index),
                       int(self.zero_correlation_zone), int(self.restricted_set), int(self.start_preamble_index),
                       int(self.nof_preamble_indices), int(self.nof_rx_ports), int(bool(self.combine_symbols)),
                       int(self.idft_size), float(self.threshold), int(self.win_margin))


@dataclass
class PrachGeometry:
    """What the detector derives from a configuration."""
    L_ra: int
    N_cs: int
    nof_shifts: int
    nof_sequences: int
    win_width: int
    max_delay_samples: int
    nof_symbols: int
    idft_size: int
    nof_elements: int


def prach_geometry(config):
    """Validates `config` as the detect calls do (ValueError) and returns its geometry; needs no device."""
    g = _Geometry()
    c = config._c()
    _lib.check(_L().srs_amd_prach_get_geometry(ctypes.byref(c), ctypes.byref(g)), "PRACH geometry")
    return PrachGeometry(*(int(getattr(g, n)) for n, _ in _Geometry._fields_))


def prach_physical_root(L_ra, logical_root_index):
    """Sequence number u of a logical root index (TS 38.211 Tables 6.3.3.1-3 / -4); needs no device."""
    u = int(_L().srs_amd_prach_physical_root(int(L_ra), int(logical_root_index)))
    if u == 0:
        raise ValueError("L_ra must be 839 or 139")
    return u


@dataclass
class PrachPreambleIndication:
    preamble_index: int
    delay_samples: int
    time_advance_s: float
    detection_metric: float
    preamble_power_db: float


@dataclass
class PrachDetectionResult:
    """prach_detection_result, plus the dense per-preamble view (the reference's log_all_opportunities)."""
    rssi_db: float
    time_resolution_s: float
    time_advance_max_s: float
    preambles: List[PrachPreambleIndication] = field(default_factory=list)
    peak_over_threshold: np.ndarray = None  # float32 [64], NaN outside the requested range
    delay_samples: np.ndarray = None        # int32 [64], -1 outside the requested range

    @staticmethod
    def _from_c(r):
        pre = [PrachPreambleIndication(int(p.preamble_index), int(p.delay_samples), float(p.time_advance_s),
                                       float(p.detection_metric), float(p.preamble_power_db))
               for p in r.preambles[:r.nof_detected]]
        return PrachDetectionResult(float(r.rssi_db), float(r.time_resolution_s), float(r.time_advance_max_s), pre,
                                    np.array([w.peak_over_threshold for w in r.windows], np.float32),
                                    np.array([w.delay_samples for w in r.windows], np.int32))


def to_cbf16(x):
    """complex array -> uint16 [..., 2] bf16 bit patterns (real, imaginary), round half to even."""
    f = np.stack([np.real(x), np.imag(x)], axis=-1).astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


class PrachBatch:
    """The configurations and buffer offsets of a batch in the C layout, validated once (ValueError)."""

    def __init__(self, configs, offsets=None):
        self.n = len(configs)
        geos = [prach_geometry(c) for c in configs]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum([g.nof_elements for g in geos])[:-1]]) if self.n else []
        offsets = [int(o) for o in offsets]
        if len(offsets) != self.n or any(o < 0 for o in offsets):
            raise ValueError("one non-negative offset per occasion")
        self.nof_elements = max([o + g.nof_elements for o, g in zip(offsets, geos)], default=0)
        self.cfgs = (_Config * max(self.n, 1))(*[c._c() for c in configs])
        self.offs = (ctypes.c_uint64 * max(self.n, 1))(*offsets)


class PrachDetector:
    """``prach_detector`` (prach_detector_generic_impl) on the GPU, any number of occasions per call."""

    def __init__(self, device=-1):
        self._lib = _L()
        h = ctypes.c_void_p()
        _lib.check(self._lib.srs_amd_prach_detector_create(ctypes.byref(h), int(device)), "PRACH detector create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srs_amd_prach_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def detect(self, symbols, config):
        """Host form, one occasion.  symbols: uint16 [ports, symbols, L_ra, 2] cbf16 bit patterns, or a complex
        [ports, symbols, L_ra] array (rounded to bf16 first)."""
        x = np.asarray(symbols)
        if np.iscomplexobj(x):
            x = to_cbf16(x)
        x = np.ascontiguousarray(x, np.uint16)
        g = prach_geometry(config)
        if x.size != 2 * g.nof_elements:
            raise ValueError("symbols hold %d values, the occasion needs %d x 2" % (x.size, g.nof_elements))
        c, r = config._c(), _Result()
        _lib.check(self._lib.srs_amd_prach_detect(self._h, ctypes.byref(c), x.ctypes.data, ctypes.byref(r)),
                   "PRACH detect")
        return PrachDetectionResult._from_c(r)

    def detect_batch(self, symbols, configs, offsets=None, results=None, stream=None):
        """Device form, asynchronous.  symbols: one contiguous device tensor holding every occasion's cbf16 values
        (int16 / uint16 / bfloat16 with the (re, im) pairs innermost, or int32 / uint32 words); configs: a list of
        PrachConfiguration with offsets per occasion in cbf16 elements (default: packed back to back), or a
        PrachBatch prepared once for a static cell configuration.  Returns the device tensor of raw results
        (uint8 [n, RESULT_BYTES]); read it with results_to_host()."""
        import torch

        if not symbols.is_cuda or not symbols.is_contiguous():
            raise ValueError("symbols must be a contiguous device tensor")
        batch = configs if isinstance(configs, PrachBatch) else PrachBatch(configs, offsets)
        n = batch.n
        if batch.nof_elements > symbols.numel() * symbols.element_size() // 4:
            raise ValueError("the occasions need %d cbf16 elements, the buffer holds %d"
                             % (batch.nof_elements, symbols.numel() * symbols.element_size() // 4))
        if results is None:
            results = torch.empty((n, RESULT_BYTES), dtype=torch.uint8, device=symbols.device)
        elif (results.dtype != torch.uint8 or not results.is_contiguous() or results.numel() < n * RESULT_BYTES
              or results.device != symbols.device):
            raise ValueError("results must be a contiguous uint8 device tensor of n x RESULT_BYTES")
        if stream is None:
            stream = torch.cuda.current_stream(symbols.device)
        _lib.check(self._lib.srs_amd_prach_detect_batch(self._h, batch.cfgs, n, symbols.data_ptr(), batch.offs,
                                                        results.data_ptr(), ctypes.c_void_p(stream.cuda_stream)),
                   "PRACH detect batch")
        return results

    @staticmethod
    def results_to_host(results):
        """Device results of detect_batch -> list of PrachDetectionResult (synchronises on the copy)."""
        raw = results.cpu().numpy().reshape(-1, RESULT_BYTES)
        return [PrachDetectionResult._from_c(_Result.from_buffer_copy(raw[i].tobytes())) for i in range(raw.shape[0])]
