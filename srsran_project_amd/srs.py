"""Host-side mirror of srsRAN's SRS channel estimator over the MI355X C-ABI (include/srsran_amd/srs.h).

Reference interfaces:
  srs_estimator.h                  estimate(const resource_grid_reader& grid, const srs_estimator_configuration& config)
  srs_estimator_configuration.h    srs_estimator_configuration (slot, srs_resource_configuration, ports)
  srs_estimator_result.h:32        srs_estimator_result

The reference reports DBL_MIN as the lower time-alignment bound (a max() over an initialiser that is the smallest
positive double); ``ta_min_s`` here is ``-ta_max_s``.
"""
import ctypes
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from . import _lib

MAX_PORTS = 4
NSYMB = 14


class _Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "nof_antenna_ports", "nof_symbols", "start_symbol", "configuration_index", "sequence_id", "bandwidth_index",
        "comb_size", "comb_offset", "cyclic_shift", "freq_position", "freq_shift", "freq_hopping", "hopping",
        "numerology", "nof_rx_ports")] + [
        ("rx_ports", ctypes.c_uint8 * MAX_PORTS), ("grid", ctypes.c_uint32), ("d_grid", ctypes.c_void_p)]


class _Information(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "sequence_length", "sequence_group", "sequence_number", "n_cs", "n_cs_max", "mapping_initial_subcarrier",
        "comb_size", "idft_size")]


class _Result(ctypes.Structure):
    _fields_ = [("channel_matrix", ((ctypes.c_float * 2) * MAX_PORTS) * MAX_PORTS),
                ("epre_db", ctypes.c_float), ("rsrp_db", ctypes.c_float), ("noise_variance", ctypes.c_float),
                ("reserved", ctypes.c_uint32),
                ("time_alignment_s", ctypes.c_double), ("ta_resolution_s", ctypes.c_double),
                ("ta_min_s", ctypes.c_double), ("ta_max_s", ctypes.c_double)]


RESULT_BYTES = ctypes.sizeof(_Result)

_declared = False


def _L():
    global _declared
    lib = _lib.lib()
    if not _declared:
        c, P = ctypes, ctypes.c_void_p
        U = c.c_uint32
        for name, res, args in [
            ("srs_amd_srs_estimator_create", c.c_int, [c.POINTER(P), c.c_int]),
            ("srs_amd_srs_estimator_destroy", None, [P]),
            ("srs_amd_srs_bandwidth", c.c_int, [U, U, c.POINTER(U), c.POINTER(U)]),
            ("srs_amd_srs_get_information", c.c_int, [c.POINTER(_Config), U, c.POINTER(_Information)]),
            ("srs_amd_srs_validate", c.c_int, [c.POINTER(_Config), U, U]),
            ("srs_amd_srs_estimate", c.c_int, [P, c.POINTER(_Config), P, U, U, c.POINTER(_Result)]),
            ("srs_amd_srs_estimate_batch", c.c_int, [P, c.POINTER(_Config), U, P, c.c_uint64, U, U, U, P, P]),
        ]:
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _declared = True
    return lib


@dataclass
class SrsConfiguration:
    """srs_estimator_configuration: the fields of srs_resource_configuration, the slot numerology and the receive
    port list.  ``grid`` selects the grid of a batch; ``d_grid`` (a device pointer) gives the PDU a grid of its own."""
    nof_antenna_ports: int
    nof_symbols: int
    start_symbol: int
    configuration_index: int
    sequence_id: int
    bandwidth_index: int
    comb_size: int
    comb_offset: int
    cyclic_shift: int
    freq_position: int = 0
    freq_shift: int = 0
    freq_hopping: int = 0
    hopping: int = 0
    numerology: int = 1
    rx_ports: Sequence[int] = field(default_factory=lambda: [0])
    grid: int = 0
    d_grid: int = 0

    def _c(self):
        ports = [int(p) for p in self.rx_ports]
        if any(p < 0 or p > 255 for p in ports):
            raise ValueError("rx ports must be in 0..255")
        arr = (ctypes.c_uint8 * MAX_PORTS)(*ports[:MAX_PORTS])
        return _Config(int(self.nof_antenna_ports), int(self.nof_symbols), int(self.start_symbol),
                       int(self.configuration_index), int(self.sequence_id), int(self.bandwidth_index),
                       int(self.comb_size), int(self.comb_offset), int(self.cyclic_shift), int(self.freq_position),
                       int(self.freq_shift), int(self.freq_hopping), int(self.hopping), int(self.numerology),
                       len(ports), arr, int(self.grid), ctypes.c_void_p(int(self.d_grid) or None))


@dataclass
class SrsInformation:
    """srs_information of one antenna port, plus the IDFT size of the time-alignment stage."""
    sequence_length: int
    sequence_group: int
    sequence_number: int
    n_cs: int
    n_cs_max: int
    mapping_initial_subcarrier: int
    comb_size: int
    idft_size: int


def srs_information(config, antenna_port=0):
    """get_srs_information of `antenna_port`; validates the resource as the estimate calls do (ValueError).  Needs no
    device."""
    info = _Information()
    c = config._c()
    _lib.check(_L().srs_amd_srs_get_information(ctypes.byref(c), int(antenna_port), ctypes.byref(info)),
               "SRS information")
    return SrsInformation(*(int(getattr(info, n)) for n, _ in _Information._fields_))


def srs_bandwidth(c_srs, b_srs):
    """(m_SRS, N) of TS 38.211 Table 6.4.1.4.3-1; ValueError outside the table.  Needs no device."""
    if c_srs < 0 or b_srs < 0:
        raise ValueError("negative index")
    m, n = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(_L().srs_amd_srs_bandwidth(int(c_srs), int(b_srs), ctypes.byref(m), ctypes.byref(n)), "SRS bandwidth")
    return int(m.value), int(n.value)


def srs_validate(config, nof_grid_ports, nof_subc):
    """The whole validation of the estimate calls for one PDU (ValueError).  Needs no device."""
    c = config._c()
    _lib.check(_L().srs_amd_srs_validate(ctypes.byref(c), int(nof_grid_ports), int(nof_subc)), "SRS validation")


@dataclass
class SrsEstimationResult:
    """srs_estimator_result."""
    channel_matrix: np.ndarray  # complex64 [nof_rx_ports, nof_antenna_ports], divided by the noise standard deviation
    epre_db: float
    rsrp_db: float
    noise_variance: float
    time_alignment_s: float
    ta_resolution_s: float
    ta_min_s: float
    ta_max_s: float

    @staticmethod
    def _from_c(r, nof_rx_ports=MAX_PORTS, nof_antenna_ports=MAX_PORTS):
        m = np.ctypeslib.as_array(r.channel_matrix).reshape(MAX_PORTS, MAX_PORTS, 2).astype(np.float32)
        m = (m[..., 0] + 1j * m[..., 1]).astype(np.complex64)[:nof_rx_ports, :nof_antenna_ports]
        return SrsEstimationResult(m, float(np.float32(r.epre_db)), float(np.float32(r.rsrp_db)),
                                   float(np.float32(r.noise_variance)), float(r.time_alignment_s),
                                   float(r.ta_resolution_s), float(r.ta_min_s), float(r.ta_max_s))


class SrsBatch:
    """The configurations of a batch in the C layout, converted once (a cell's SRS resources are static)."""

    def __init__(self, configs):
        self.configs = list(configs)
        self.n = len(self.configs)
        self.cfgs = (_Config * max(self.n, 1))(*[c._c() for c in self.configs])


class SrsEstimator:
    """``srs_estimator`` (srs_estimator_generic_impl) on the GPU, any number of PDUs per call."""

    def __init__(self, device=-1):
        self._lib = _L()
        h = ctypes.c_void_p()
        _lib.check(self._lib.srs_amd_srs_estimator_create(ctypes.byref(h), int(device)), "SRS estimator create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srs_amd_srs_estimator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, grid, config):
        """Host form, one PDU.  grid: uint16 [ports, 14, nof_subc, 2] cbf16 bit patterns (numpy)."""
        x = np.ascontiguousarray(grid, np.uint16)
        if x.ndim != 4 or x.shape[1] != NSYMB or x.shape[3] != 2:
            raise ValueError("grid must be uint16 [ports, 14, nof_subc, 2]")
        c, r = config._c(), _Result()
        _lib.check(self._lib.srs_amd_srs_estimate(self._h, ctypes.byref(c), x.ctypes.data, x.shape[0], x.shape[2],
                                                  ctypes.byref(r)), "SRS estimate")
        return SrsEstimationResult._from_c(r, len(config.rx_ports), config.nof_antenna_ports)

    def estimate_batch(self, grids, configs, results=None, stream=None):
        """Device form, asynchronous.  grids: a contiguous device tensor [nof_grids, ports, 14, nof_subc, 2] of cbf16
        halves (int16 / uint16 / bfloat16); configs: a list of SrsConfiguration whose ``grid`` selects the grid, or an
        SrsBatch prepared once.  Returns the device tensor of raw results (uint8 [n, RESULT_BYTES]); read it with results_to_host()."""
        import torch

        if not grids.is_cuda or not grids.is_contiguous():
            raise ValueError("grids must be a contiguous device tensor")
        if grids.dim() != 5 or grids.shape[2] != NSYMB or grids.shape[4] != 2 or grids.element_size() != 2:
            raise ValueError("grids must be [nof_grids, ports, 14, nof_subc, 2] of 16-bit values")
        batch = configs if isinstance(configs, SrsBatch) else SrsBatch(configs)
        n, cfgs = batch.n, batch.cfgs
        nof_grids, nof_ports, nof_subc = int(grids.shape[0]), int(grids.shape[1]), int(grids.shape[3])
        if results is None:
            results = torch.empty((n, RESULT_BYTES), dtype=torch.uint8, device=grids.device)
        elif (results.dtype != torch.uint8 or not results.is_contiguous() or results.numel() < n * RESULT_BYTES
              or results.device != grids.device):
            raise ValueError("results must be a contiguous uint8 device tensor of n x RESULT_BYTES")
        if stream is None:
            stream = torch.cuda.current_stream(grids.device)
        _lib.check(self._lib.srs_amd_srs_estimate_batch(self._h, cfgs, n, grids.data_ptr(),
                                                        nof_ports * NSYMB * nof_subc, nof_grids, nof_ports, nof_subc,
                                                        results.data_ptr(), ctypes.c_void_p(stream.cuda_stream)),
                   "SRS estimate batch")
        return results

    @staticmethod
    def results_to_host(results, configs=None):
        """Device results of estimate_batch -> list of SrsEstimationResult (synchronises on the copy); with the
        configurations the matrices are cut to [nof_rx_ports, nof_antenna_ports]."""
        raw = results.cpu().numpy().reshape(-1, RESULT_BYTES)
        if isinstance(configs, SrsBatch):
            configs = configs.configs
        out = []
        for i in range(raw.shape[0]):
            r = _Result.from_buffer_copy(raw[i].tobytes())
            if configs is not None:
                out.append(SrsEstimationResult._from_c(r, len(configs[i].rx_ports), configs[i].nof_antenna_ports))
            else:
                out.append(SrsEstimationResult._from_c(r))
        return out
