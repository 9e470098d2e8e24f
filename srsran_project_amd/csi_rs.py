"""Host-side mirror of srsRAN's NZP-CSI-RS generator over the MI355X C-ABI (include/srsran_amd/csi_rs.h).

Reference interfaces:
  nzp_csi_rs_generator.h:88     map(resource_grid_writer& grid, const config_t& config)
  nzp_csi_rs_generator.h:46-80  config_t (slot, start_rb, nof_rb, csi_rs_mapping_table_row, freq_allocation_ref_idx,
                                symbol_l0, symbol_l1, cdm, freq_density, scrambling_id, amplitude, precoding)
  csi_rs_pattern.h              get_csi_rs_pattern(const csi_rs_pattern_configuration&)

Grids are cbf16 bit patterns: uint16 [ports, 14, nof_subc, 2] (re, im) on the host, a contiguous 16-bit device tensor
[nof_grids, ports, 14, nof_subc, 2] for the slot form.  Mapping covers rows 1-5; the pattern helpers rows 1-12.
"""
import ctypes
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from . import _lib
from .pdsch_modulator import MAX_PATTERNS, RePattern, ReservedPattern

MAX_PORTS = 4
MAX_PATTERN_PORTS = 16
MAX_K_REF = 6
NSYMB = 14

CDM_NONE, CDM_FD2, CDM_FD2_TD2, CDM_FD2_TD4 = 0, 1, 2, 3
DENSITY_THREE, DENSITY_ONE, DENSITY_DOT5_EVEN, DENSITY_DOT5_ODD = 0, 1, 2, 3


class _Config(ctypes.Structure):
    _fields_ = [("numerology", ctypes.c_uint32), ("slot_index", ctypes.c_uint32), ("start_rb", ctypes.c_uint32),
                ("nof_rb", ctypes.c_uint32), ("row", ctypes.c_uint32), ("nof_k_ref", ctypes.c_uint32),
                ("k_ref", ctypes.c_uint32 * MAX_K_REF), ("symbol_l0", ctypes.c_uint32),
                ("symbol_l1", ctypes.c_uint32), ("cdm", ctypes.c_uint32), ("freq_density", ctypes.c_uint32),
                ("scrambling_id", ctypes.c_uint32), ("amplitude", ctypes.c_float),
                ("weights", ctypes.c_float * (MAX_PORTS * MAX_PORTS * 2)), ("grid", ctypes.c_uint32),
                ("d_grid", ctypes.c_void_p)]


class _PatternPort(ctypes.Structure):
    _fields_ = [("re_mask", ctypes.c_uint16), ("symbol_mask", ctypes.c_uint16)]


class _Pattern(ctypes.Structure):
    _fields_ = [("rb_begin", ctypes.c_uint32), ("rb_end", ctypes.c_uint32), ("rb_stride", ctypes.c_uint32),
                ("nof_ports", ctypes.c_uint32), ("port", _PatternPort * MAX_PATTERN_PORTS)]


_declared = False


def _L():
    global _declared
    lib = _lib.lib()
    if not _declared:
        c, P = ctypes, ctypes.c_void_p
        U = c.c_uint32
        for name, res, args in [
            ("srs_amd_csi_rs_generator_create", c.c_int, [c.POINTER(P), c.c_int]),
            ("srs_amd_csi_rs_generator_destroy", None, [P]),
            ("srs_amd_csi_rs_pattern", c.c_int, [c.POINTER(_Config), c.POINTER(_Pattern)]),
            ("srs_amd_csi_rs_reserved", c.c_int, [c.POINTER(_Config), c.POINTER(RePattern), c.POINTER(U)]),
            ("srs_amd_csi_rs_validate", c.c_int, [c.POINTER(_Config), U, U]),
            ("srs_amd_csi_rs_map", c.c_int, [P, c.POINTER(_Config), P, U, U]),
            ("srs_amd_csi_rs_map_slot", c.c_int, [P, c.POINTER(_Config), U, P, c.c_uint64, U, U, U, P]),
        ]:
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _declared = True
    return lib


@dataclass
class CsiRsConfig:
    """nzp_csi_rs_generator::config_t.  ``weights``: complex [CSI-RS port][tx port] for the whole band (None: the
    identity); ``grid`` selects the grid of a slot call, ``d_grid`` (a device pointer) gives the resource a grid of its
    own."""
    row: int
    k_ref: Sequence[int]
    symbol_l0: int
    start_rb: int
    nof_rb: int
    cdm: int = CDM_NONE
    freq_density: int = DENSITY_ONE
    scrambling_id: int = 0
    amplitude: float = 1.0
    numerology: int = 1
    slot_index: int = 0
    symbol_l1: int = 0
    weights: object = None
    grid: int = 0
    d_grid: int = 0

    def _c(self):
        k = [int(v) for v in self.k_ref]
        fields = (self.row, self.symbol_l0, self.symbol_l1, self.start_rb, self.nof_rb, self.cdm, self.freq_density,
                  self.scrambling_id, self.numerology, self.slot_index, self.grid, *k)
        if any(int(v) < 0 or int(v) > 0xFFFFFFFF for v in fields):
            raise ValueError("CSI-RS configuration field out of range")
        c = _Config()
        c.numerology, c.slot_index = int(self.numerology), int(self.slot_index)
        c.start_rb, c.nof_rb, c.row = int(self.start_rb), int(self.nof_rb), int(self.row)
        c.nof_k_ref = len(k)
        for i, v in enumerate(k[:MAX_K_REF]):
            c.k_ref[i] = v
        c.symbol_l0, c.symbol_l1 = int(self.symbol_l0), int(self.symbol_l1)
        c.cdm, c.freq_density, c.scrambling_id = int(self.cdm), int(self.freq_density), int(self.scrambling_id)
        c.amplitude = float(self.amplitude)
        w = np.eye(MAX_PORTS, dtype=np.complex64)
        if self.weights is not None:
            given = np.asarray(self.weights, np.complex64)
            if given.ndim != 2 or given.shape[0] > MAX_PORTS or given.shape[1] > MAX_PORTS:
                raise ValueError("weights must be complex [CSI-RS port][tx port], at most 4 x 4")
            w = np.zeros((MAX_PORTS, MAX_PORTS), np.complex64)
            w[:given.shape[0], :given.shape[1]] = given
        flat = np.stack([w.real, w.imag], axis=-1).astype(np.float32).ravel()
        c.weights = (ctypes.c_float * flat.size)(*flat.tolist())
        c.grid = int(self.grid)
        c.d_grid = ctypes.c_void_p(int(self.d_grid) or None)
        return c


@dataclass
class CsiRsPattern:
    """csi_rs_pattern: PRBs rb_begin, rb_begin + rb_stride, ... < rb_end; per port a 12-bit RE mask and a 14-bit symbol
    mask."""
    rb_begin: int
    rb_end: int
    rb_stride: int
    re_masks: list = field(default_factory=list)
    symbol_masks: list = field(default_factory=list)

    @property
    def nof_ports(self):
        return len(self.re_masks)


def csi_rs_pattern(config):
    """get_csi_rs_pattern for rows 1-12 (ValueError where the reference asserts).  Needs no device."""
    c, p = config._c(), _Pattern()
    _lib.check(_L().srs_amd_csi_rs_pattern(ctypes.byref(c), ctypes.byref(p)), "CSI-RS pattern")
    n = int(p.nof_ports)
    return CsiRsPattern(int(p.rb_begin), int(p.rb_end), int(p.rb_stride), [int(p.port[i].re_mask) for i in range(n)],
                        [int(p.port[i].symbol_mask) for i in range(n)])


def csi_rs_reserved(config):
    """The REs of the resource as ReservedPattern entries, one per CDM group with distinct REs, ready for
    PdschModulatorConfig.reserved.  Needs no device."""
    c = config._c()
    pats = (RePattern * MAX_PATTERNS)()
    n = ctypes.c_uint32()
    _lib.check(_L().srs_amd_csi_rs_reserved(ctypes.byref(c), pats, ctypes.byref(n)), "CSI-RS reserved")
    out = []
    for i in range(int(n.value)):
        mask = bytes(pats[i].crb_mask)
        crbs = [r for r in range(8 * len(mask)) if (mask[r // 8] >> (r % 8)) & 1]
        out.append(ReservedPattern(crbs, int(pats[i].re_mask), int(pats[i].symbols)))
    return out


def csi_rs_validate(config, nof_grid_ports, nof_subc):
    """Everything the map calls check for one resource (ValueError).  Needs no device."""
    c = config._c()
    _lib.check(_L().srs_amd_csi_rs_validate(ctypes.byref(c), int(nof_grid_ports), int(nof_subc)), "CSI-RS validation")


class CsiRsBatch:
    """The configurations of a slot call in the C layout, converted once (a cell's CSI-RS resources are static)."""

    def __init__(self, configs):
        self.configs = list(configs)
        self.n = len(self.configs)
        self.cfgs = (_Config * max(self.n, 1))(*[c._c() for c in self.configs])


class CsiRsGenerator:
    """``nzp_csi_rs_generator`` (nzp_csi_rs_generator_impl) on the GPU, any number of resources per call."""

    def __init__(self, device=-1):
        self._lib = _L()
        h = ctypes.c_void_p()
        _lib.check(self._lib.srs_amd_csi_rs_generator_create(ctypes.byref(h), int(device)), "CSI-RS generator create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srs_amd_csi_rs_generator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def map(self, grid, config):
        """Host form, one resource.  grid: uint16 [ports, 14, nof_subc, 2] cbf16 bit patterns (numpy); returns the
        grid with the resource mapped, every other RE as given."""
        x = np.array(grid, dtype=np.uint16, order="C")
        if x.ndim != 4 or x.shape[1] != NSYMB or x.shape[3] != 2:
            raise ValueError("grid must be uint16 [ports, 14, nof_subc, 2]")
        c = config._c()
        _lib.check(self._lib.srs_amd_csi_rs_map(self._h, ctypes.byref(c), x.ctypes.data, x.shape[0], x.shape[2]),
                   "CSI-RS map")
        return x

    def map_slot(self, grids, configs, stream=None):
        """Device form, asynchronous, one kernel launch.  grids: a contiguous device tensor
        [nof_grids, ports, 14, nof_subc, 2] of cbf16 halves (int16 / uint16 / bfloat16), updated in place; configs: a
        list of CsiRsConfig whose ``grid`` selects the grid (or whose ``d_grid`` points to a grid of the same shape), or
        a CsiRsBatch prepared once."""
        import torch

        if not grids.is_cuda or not grids.is_contiguous():
            raise ValueError("grids must be a contiguous device tensor")
        if grids.dim() != 5 or grids.shape[2] != NSYMB or grids.shape[4] != 2 or grids.element_size() != 2:
            raise ValueError("grids must be [nof_grids, ports, 14, nof_subc, 2] of 16-bit values")
        batch = configs if isinstance(configs, CsiRsBatch) else CsiRsBatch(configs)
        n, cfgs = batch.n, batch.cfgs
        nof_grids, nof_ports, nof_subc = int(grids.shape[0]), int(grids.shape[1]), int(grids.shape[3])
        if stream is None:
            stream = torch.cuda.current_stream(grids.device)
        _lib.check(self._lib.srs_amd_csi_rs_map_slot(self._h, cfgs, n, grids.data_ptr(), nof_ports * NSYMB * nof_subc,
                                                     nof_grids, nof_ports, nof_subc,
                                                     ctypes.c_void_p(stream.cuda_stream)), "CSI-RS map slot")
        return grids
