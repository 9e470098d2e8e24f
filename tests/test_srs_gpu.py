"""SRS channel estimator on the MI355X (srs_amd_srs_estimate / srs_amd_srs_estimate_batch through the Python layer).

References: the fixtures recorded from the reference's own estimator (tests/golden/srs_golden.npz, written by
tools/srs_golden_gen.cpp) and the float64 model (tests/srs_model.py).  The GPU is never compared with itself for
accuracy; the batch / stream tests compare raw results of the same deterministic kernels for identity.

Every grid the GPU sees is the 14-symbol grid built around the recorded rows: seeded non-zero garbage in every other
symbol, in the ports the PDU does not list and on the subcarriers of the SRS symbols it does not use.

Exact: the integer correlation peak (round(TA / resolution) for one antenna port; with several ports the result
holds only their mean, and a wrong tap in any port would move it by at least a quarter of a sample, 1e5 times the
bound below), ta_resolution_s and ta_max_s within half a T_c, ta_min_s = -ta_max_s, the NaN / inf class of every
field on the all-zero grid, zeros in the unused matrix entries.

Tolerances of the float fields.  Measured on the fixtures, the reference (float32) deviates from the float64 model by
at most
    channel matrix     7.62e-6 of the Frobenius norm of the case's matrix
    noise_variance     2.53e-5 relative
    epre_db            1.92e-6 dB
    rsrp_db            1.42e-5 dB
    time alignment     3.52e-7 IDFT samples (the fractional tap)
(tests/test_srs_model.py prints them; sm.reference_deviation() recomputes them here).  The GPU is float32 too, with
another, equally valid summation and DFT order, and gets four times that -- the margin this project chose for PRACH:
3.05e-5, 1.01e-4, 7.7e-6 dB, 5.67e-5 dB, 1.41e-6 samples, against the fixtures and against the model.
"""
import math

import numpy as np
import pytest

from tests import srs_model as sm

pytestmark = pytest.mark.gpu

FIXTURES = sm.fixtures()
IDS = [fx.name for fx in FIXTURES]
T_C = sm.T_C
_DEV = sm.reference_deviation()
TOL_COEF, TOL_NV, TOL_EPRE_DB, TOL_RSRP_DB, TOL_TA = (4.0 * v for v in _DEV)
BATCH_PORTS, BATCH_SUBC = 4, 3300


def test_tolerances_are_the_documented_ones():
    assert abs(TOL_COEF - 3.05e-5) < 0.005e-5 and abs(TOL_NV - 1.01e-4) < 0.005e-4
    assert abs(TOL_EPRE_DB - 7.7e-6) < 0.05e-6 and abs(TOL_RSRP_DB - 5.67e-5) < 0.005e-5
    assert abs(TOL_TA - 1.41e-6) < 0.005e-6


@pytest.fixture(scope="module")
def estimator(device):
    import srsran_project_amd as amd

    est = amd.SrsEstimator(device.index or 0)
    yield est
    est.close()


def _value_class(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("+inf" if v > 0 else "-inf") if math.isinf(v) else "finite"


def _check_fields(res, matrix, epre_db, rsrp_db, nv, ta, resolution, label, what):
    norm = np.linalg.norm(matrix)
    dev = (np.abs(res.channel_matrix - matrix).max() / norm, abs(res.noise_variance - nv) / nv,
           abs(res.epre_db - epre_db), abs(res.rsrp_db - rsrp_db), abs(res.time_alignment_s - ta) / resolution)
    print("%s from the %s: coefficients %.3e of the norm, noise variance %.3e relative, epre %.3e dB, rsrp %.3e dB, "
          "time alignment %.3e samples" % ((label, what) + dev))
    assert dev[0] <= TOL_COEF and dev[1] <= TOL_NV and dev[2] <= TOL_EPRE_DB and dev[3] <= TOL_RSRP_DB, (label, what)
    assert dev[4] <= TOL_TA, (label, what)


def _check_against_model(res, m, cfg, label):
    assert res.channel_matrix.shape == (len(cfg.rx_ports), cfg.nof_antenna_ports)
    assert abs(res.ta_resolution_s - m["ta_resolution_s"]) < 0.5 * T_C
    assert abs(res.ta_max_s - m["ta_max_s"]) < 0.5 * T_C
    assert res.ta_min_s == -res.ta_max_s
    if cfg.nof_antenna_ports == 1:
        assert round(res.time_alignment_s / res.ta_resolution_s) == m["idx_ports"][0], label
    _check_fields(res, m["matrix"], m["epre_db"], m["rsrp_db"], m["noise_variance"], m["time_alignment_s"],
                  m["ta_resolution_s"], label, "model")


def _check_fixture(res, fx):
    assert abs(res.ta_resolution_s - fx.ta_resolution_s) < 0.5 * T_C
    assert abs(res.ta_max_s - fx.ta_max_s) < 0.5 * T_C
    assert res.ta_min_s == -res.ta_max_s
    if fx.all_zero:
        got = [res.channel_matrix.real, res.channel_matrix.imag, res.epre_db, res.rsrp_db, res.noise_variance,
               res.time_alignment_s]
        ref = [fx.matrix.real, fx.matrix.imag, fx.epre_db, fx.rsrp_db, fx.noise_variance, fx.time_alignment_s]
        for g, r in zip(got, ref):
            assert [_value_class(v) for v in np.ravel(g)] == [_value_class(v) for v in np.ravel(r)], fx.name
        return
    if fx.cfg.nof_antenna_ports == 1:
        assert round(res.time_alignment_s / res.ta_resolution_s) == round(fx.time_alignment_s / fx.ta_resolution_s)
    _check_fields(res, fx.matrix.astype(np.complex128), float(fx.epre_db), float(fx.rsrp_db), float(fx.noise_variance),
                  fx.time_alignment_s, fx.ta_resolution_s, fx.name, "reference")
    _check_against_model(res, fx.model(), fx.cfg, fx.name)


def _raw_matrix_is_zero_outside(raw_row, cfg):
    import srsran_project_amd as amd

    m = np.frombuffer(raw_row.tobytes()[:128], np.float32).reshape(4, 4, 2)
    used = np.zeros((4, 4), bool)
    used[:len(cfg.rx_ports), :cfg.nof_antenna_ports] = True
    assert amd.srs.RESULT_BYTES == 176
    return not m[~used].view(np.uint32).any()


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_host_form(estimator, fx):
    # one grid port more than the highest listed one, the fixture's own (mostly odd) number of subcarriers
    grid = sm.build_grid(fx.x, fx.cfg, max(fx.cfg.rx_ports) + 2, 1000 + len(fx.name))
    _check_fixture(estimator.estimate(grid, fx.cfg.library()), fx)


def test_fixtures_one_heterogeneous_batch(estimator, device):
    import torch

    grids = np.stack([sm.build_grid(fx.x, fx.cfg, BATCH_PORTS, 2000 + i, nof_subc=BATCH_SUBC)
                      for i, fx in enumerate(FIXTURES)])
    cfgs = [fx.cfg.library(grid=i) for i, fx in enumerate(FIXTURES)]
    raw = estimator.estimate_batch(torch.from_numpy(grids.view(np.int16)).to(device), cfgs)
    torch.cuda.synchronize()
    rows = raw.cpu().numpy()
    for i, (res, fx) in enumerate(zip(estimator.results_to_host(raw, cfgs), FIXTURES)):
        _check_fixture(res, fx)
        assert _raw_matrix_is_zero_outside(rows[i], fx.cfg), fx.name


# ---- fresh seeded inputs against the float64 model ---------------------------------------------------------------

class Fresh:
    def __init__(self, name, nof_grid_ports, nof_subc, delay, sigma, seed, **cfg):
        self.name, self.nof_grid_ports, self.nof_subc = name, nof_grid_ports, nof_subc
        self.cfg = sm.Config(**cfg)
        rng = np.random.default_rng(seed)
        self.x = sm.make_rows(rng, self.cfg, nof_subc, delay, sigma)
        self.grid = sm.build_grid(self.x, self.cfg, nof_grid_ports, seed + 500)
        self._model = None

    def model(self):
        if self._model is None:
            self._model = sm.estimate(sm.from_cbf16(self.x), self.cfg)
        return self._model


_fresh = None


def fresh_cases():
    """Shapes the fixtures do not hold: three rx ports, odd numbers of subcarriers, grids with more ports than the PDU
    lists, the 512-point kernel with four symbols, interleaved pilots over three rx ports, a length-36 sequence.
    Built once."""
    global _fresh
    if _fresh is None:
        base = dict(freq_position=0, freq_hopping=0)
        _fresh = [
            Fresh("m72_comb2_2x3_ports310", 5, 301, 0.3, 0.5, 1, nof_antenna_ports=2, nof_symbols=2, start_symbol=3,
                  configuration_index=2, sequence_id=77, bandwidth_index=0, comb_size=2, comb_offset=1,
                  cyclic_shift=5, freq_shift=11, numerology=1, rx_ports=[3, 1, 0], **base),
            Fresh("m264_comb4_4x3_cs_high", 4, 1077, -0.45, 0.6, 2, nof_antenna_ports=4, nof_symbols=1,
                  start_symbol=13, configuration_index=22, sequence_id=401, bandwidth_index=0, comb_size=4,
                  comb_offset=1, cyclic_shift=10, freq_shift=1, numerology=0, rx_ports=[2, 3, 0], **base),
            Fresh("m408_comb2_1x3_4sym", 8, 901, 0.65, 1.0, 3, nof_antenna_ports=1, nof_symbols=4, start_symbol=6,
                  configuration_index=34, sequence_id=1000, bandwidth_index=1, comb_size=2, comb_offset=0,
                  cyclic_shift=6, freq_shift=4, numerology=1, rx_ports=[7, 0, 4], freq_position=0, freq_hopping=2),
            Fresh("m36_comb4_2x1", 2, 165, -0.7, 0.3, 4, nof_antenna_ports=2, nof_symbols=1, start_symbol=0,
                  configuration_index=2, sequence_id=29, bandwidth_index=0, comb_size=4, comb_offset=2,
                  cyclic_shift=8, freq_shift=1, numerology=1, rx_ports=[1], freq_position=0, freq_hopping=3),
            Fresh("m1632_comb2_4x3_cs_low", 3, 3299, 0.2, 0.8, 5, nof_antenna_ports=4, nof_symbols=1, start_symbol=9,
                  configuration_index=63, sequence_id=515, bandwidth_index=0, comb_size=2, comb_offset=0,
                  cyclic_shift=1, freq_shift=2, numerology=1, rx_ports=[1, 2, 0], **base),
        ]
    return _fresh


def test_fresh_inputs_are_well_conditioned():
    """Precondition of the next tests, on the model alone."""
    for c in fresh_cases():
        assert sm.peak_margin(c.model()) >= 1.5, c.name


def test_fresh_inputs_host_form(estimator):
    for c in fresh_cases():
        _check_against_model(estimator.estimate(c.grid, c.cfg.library()), c.model(), c.cfg, c.name)


def test_fresh_inputs_own_grids_in_one_batch(estimator, device):
    """Every PDU brings its own device grid (d_grid) of the batch's shape."""
    import torch

    cases = [c for c in fresh_cases() if c.nof_grid_ports <= 5 and c.nof_subc <= 1077]
    ports, subc = 5, 1077
    dev = [torch.from_numpy(sm.build_grid(c.x, c.cfg, ports, 600 + i, nof_subc=subc).view(np.int16)).to(device)
           for i, c in enumerate(cases)]
    cfgs = [c.cfg.library(grid=99, d_grid=g.data_ptr()) for c, g in zip(cases, dev)]
    raw = estimator.estimate_batch(dev[0].reshape(1, ports, 14, subc, 2), cfgs)
    torch.cuda.synchronize()
    for res, c in zip(estimator.results_to_host(raw, cfgs), cases):
        _check_against_model(res, c.model(), c.cfg, c.name)


# ---- batch and stream behaviour ------------------------------------------------------------------------------------

def _raw(estimator, grids, cfgs, stream=None):
    import torch

    out = estimator.estimate_batch(grids, cfgs, stream=stream)
    (stream or torch.cuda.current_stream()).synchronize()
    return out.cpu().numpy()


def _shared_grid():
    """Two PDUs on one grid: the same symbols and rx ports, comb offsets 0 and 2 of comb 4, other cyclic shifts and
    sequence identities."""
    kw = dict(nof_symbols=2, start_symbol=10, configuration_index=12, bandwidth_index=0, comb_size=4, freq_shift=2,
              numerology=1, rx_ports=[2, 0])
    a = sm.Config(nof_antenna_ports=2, sequence_id=3, comb_offset=0, cyclic_shift=4, **kw)
    b = sm.Config(nof_antenna_ports=1, sequence_id=200, comb_offset=2, cyclic_shift=9, **kw)
    rng = np.random.default_rng(77)
    rows = sm.to_cbf16(sm.make_complex_rows(rng, a, 613, 0.4, 0.5) + sm.make_complex_rows(rng, b, 613, -0.3, 0.0))
    grid = sm.build_grid(rows, a, 3, 78, keep_rows=True)
    return a, b, rows, grid


def test_two_pdus_share_one_grid(estimator, device):
    import torch

    a, b, rows, grid = _shared_grid()
    grids = torch.from_numpy(grid.view(np.int16)).to(device).reshape(1, 3, 14, 613, 2)
    cfgs = [a.library(), b.library()]
    both = _raw(estimator, grids, cfgs)
    for i, c in enumerate((a, b)):
        alone = _raw(estimator, grids, [cfgs[i]])
        assert np.array_equal(alone[0], both[i])
        res = estimator.results_to_host(torch.from_numpy(both[i:i + 1]), [cfgs[i]])[0]
        _check_against_model(res, sm.estimate(sm.from_cbf16(rows), c), c, "shared grid %d" % i)


def test_results_do_not_depend_on_batch_position(estimator, device):
    import torch

    picks = [FIXTURES[i] for i in (0, 3, 5, 10, 14, 16)]
    grids = torch.from_numpy(np.stack([sm.build_grid(f.x, f.cfg, BATCH_PORTS, 3000 + i, nof_subc=BATCH_SUBC)
                                       for i, f in enumerate(picks)]).view(np.int16)).to(device)
    cfgs = [f.cfg.library(grid=i) for i, f in enumerate(picks)]
    a = _raw(estimator, grids, cfgs)
    perm = [3, 0, 5, 4, 2, 1]
    b = _raw(estimator, grids, [cfgs[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(b[j], a[i]), picks[i].name
    many = _raw(estimator, grids, [cfgs[2]] * 33 + [cfgs[4]])
    assert all(np.array_equal(many[j], a[2]) for j in range(33)) and np.array_equal(many[33], a[4])
    alone = _raw(estimator, grids, [cfgs[2]])
    assert np.array_equal(alone[0], a[2])
    for i, f in enumerate(picks):
        _check_fixture(estimator.results_to_host(torch.from_numpy(a[i:i + 1]), [cfgs[i]])[0], f)


def test_two_handles_on_two_streams(estimator, device):
    import torch

    import srsran_project_amd as amd

    first, second = FIXTURES[:8], FIXTURES[8:13]

    def pack(fxs, seed):
        g = np.stack([sm.build_grid(f.x, f.cfg, BATCH_PORTS, seed + i, nof_subc=BATCH_SUBC) for i, f in enumerate(fxs)])
        return torch.from_numpy(g.view(np.int16)).to(device), [f.cfg.library(grid=i) for i, f in enumerate(fxs)]

    g1, c1 = pack(first, 4000)
    g2, c2 = pack(second, 5000)
    want1, want2 = _raw(estimator, g1, c1), _raw(estimator, g2, c2)
    other = amd.SrsEstimator(device.index or 0)
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        outs.append((estimator.estimate_batch(g1, c1, stream=s1), other.estimate_batch(g2, c2, stream=s2)))
    # one handle used from two streams in turn: the second call waits for the first call's scratch
    o3 = estimator.estimate_batch(g2, c2, stream=s2)
    s1.synchronize()
    s2.synchronize()
    for o1, o2 in outs:
        assert np.array_equal(o1.cpu().numpy(), want1)
        assert np.array_equal(o2.cpu().numpy(), want2)
    assert np.array_equal(o3.cpu().numpy(), want2)
    other.close()


def test_second_call_hits_the_sequence_cache(device):
    """The cache is keyed by (length, group): an estimator that has served group 3 must estimate a PDU of group 4 with
    the new sequence, and group 3 again afterwards from the cache."""
    import srsran_project_amd as amd

    est = amd.SrsEstimator(device.index or 0)
    kw = dict(nof_antenna_ports=2, nof_symbols=1, start_symbol=5, configuration_index=12, bandwidth_index=0,
              comb_size=4, comb_offset=1, cyclic_shift=2, numerology=1, rx_ports=[0, 1])
    a = Fresh("cache_group3", 2, 590, 0.3, 0.5, 21, sequence_id=33, **kw)
    b = Fresh("cache_group4", 2, 590, 0.3, 0.5, 22, sequence_id=34, **kw)
    raws = []
    for c in (a, b, a):
        res = est.estimate(c.grid, c.cfg.library())
        _check_against_model(res, c.model(), c.cfg, c.name)
        raws.append(res)
    assert np.array_equal(raws[0].channel_matrix, raws[2].channel_matrix)
    assert raws[0].noise_variance == raws[2].noise_variance
    # b's grid against a's sequence holds no pilot of a's: the estimate is noise (RSRP far below the EPRE)
    cross = est.estimate(b.grid, a.cfg.library())
    assert cross.rsrp_db < cross.epre_db - 10.0
    est.close()


def test_invalid_configuration_launches_nothing(estimator, device):
    import torch

    import srsran_project_amd as amd

    fx = FIXTURES[3]
    grid = sm.build_grid(fx.x, fx.cfg, 4, 9)
    grids = torch.from_numpy(grid.view(np.int16)).to(device).reshape(1, 4, 14, fx.nof_subc, 2)
    results = torch.full((2, amd.srs.RESULT_BYTES), 0xA5, dtype=torch.uint8, device=device)
    for bad in (dict(comb_offset=4), dict(comb_size=2, comb_offset=0, cyclic_shift=8), dict(configuration_index=64),
                dict(bandwidth_index=1, freq_hopping=0), dict(hopping=1), dict(rx_ports=[]),
                dict(rx_ports=[0, 1, 2, 3, 0]), dict(rx_ports=[0, 4]), dict(start_symbol=11),
                dict(freq_shift=200), dict(nof_antenna_ports=3), dict(nof_symbols=3), dict(grid=1)):
        with pytest.raises(ValueError):
            estimator.estimate_batch(grids, [fx.cfg.library(), fx.cfg.library(**bad)], results=results)
        if "grid" not in bad:
            with pytest.raises(ValueError):
                estimator.estimate(grid, fx.cfg.library(**bad))
    torch.cuda.synchronize()
    assert bool((results == 0xA5).all())  # the valid first PDU was not launched either


def test_host_form_threads_on_one_handle_keep_their_own_input(estimator):
    """Four threads in the host form of ONE estimator, each with its own reception of the smallest fixture's PDU
    (tests/host_form_threads.py): every call returns its own thread's result bit for bit."""
    import struct

    from tests.host_form_threads import check_isolation

    fx = min(FIXTURES, key=lambda f: f.x.size)
    assert fx.name == "m12_comb4_1x1"
    cfg = fx.cfg.library()
    grids = [sm.build_grid(sm.make_rows(np.random.default_rng(7000 + i), fx.cfg, fx.nof_subc, 0.1 * (i + 1), 0.3),
                           fx.cfg, max(fx.cfg.rx_ports) + 1, 7100 + i) for i in range(4)]

    def bits(r):
        return r.channel_matrix.tobytes() + struct.pack("7d", r.epre_db, r.rsrp_db, r.noise_variance,
                                                        r.time_alignment_s, r.ta_resolution_s, r.ta_min_s, r.ta_max_s)

    check_isolation(lambda g: estimator.estimate(g, cfg), grids, bits)
