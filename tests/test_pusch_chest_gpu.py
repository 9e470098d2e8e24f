"""GPU parity: MI355X PUSCH DM-RS channel estimator (through the C-ABI) vs the
CPU oracle oracle/chest.py, itself pinned to the reference's
dmrs_pusch_estimator_impl + port_channel_estimator_average_impl
(tests/test_oracle_vs_ref.py) -- and vs the compiled reference directly when
oracle/_ref is present.  Bar (float path, sums reassociated): every bf16
estimate within two bf16 roundings (2^-6 relative) of the oracle's, stale REs
bit-exact; noise variance, EPRE, RSRP, SNR, CFO within 2e-3 relative; time
alignment within 2e-3 relative + 2 ns.  On the coherent grids (chest_cases.EDGE_CASES:
the real DM-RS with a known delay, CFO and SNR, where the noise variance is the
small residual of a coherent prediction) also: at most 1e-3 of the estimate words
differ at all, over the whole buffer and over the allocation's edge band."""
import numpy as np
import pytest

import oracle
from oracle import chest
from tests import chest_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def est():
    import srsran_project_amd as amd

    return amd.DmrsPuschEstimator(device=0)


def _config(kw):
    import srsran_project_amd as amd

    return amd.DmrsPuschEstimatorConfig(slot_index=kw["slot_index"], numerology=kw["numerology"],
                                        nof_tx_layers=kw["nof_layers"], scrambling_id=kw["scrambling_id"],
                                        n_scid=kw["n_scid"], scaling=kw["scaling"], symbols_mask=kw["symbols_mask"],
                                        rb_start=kw["prb_lo"], rb_count=kw["prb_hi"] - kw["prb_lo"],
                                        first_symbol=kw["first_symbol"], nof_symbols=kw["nof_symbols"],
                                        fd_smoothing=kw["fd"], td_interpolation=kw["td"],
                                        compensate_cfo=kw["compensate_cfo"])


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_pusch_chest_host(est, case):
    grid, kw = cc.case_args(case, seed=5)
    est0 = cc.stale_estimates(grid.shape, kw["nof_layers"], seed=7)
    want, ws = chest.pusch_chest(grid, estimates=est0, **kw)
    got, gs = est.estimate(grid, _config(kw), estimates=est0)
    cc.assert_estimates_close(got, want, case[0])
    cc.assert_stats_close(gs, ws, case[0])
    if oracle.REF is not None:
        want_r, ws_r = chest.ref_pusch_chest(grid, estimates=est0, **kw)
        cc.assert_estimates_close(got, want_r, case[0] + " vs reference")
        cc.assert_stats_close(gs, ws_r, case[0] + " vs reference")


def test_pusch_chest_batch(est):
    import torch

    case = cc.CASES[2]  # 4 rx ports, 273 PRB, 4 layers
    n = 3
    grids, kws = zip(*[cc.case_args(case, seed=s) for s in range(n)])
    kw = dict(kws[0])
    g_dev = torch.from_numpy(np.stack(grids).view(np.int32)).to("cuda:0")
    e0 = np.stack([cc.stale_estimates(grids[0].shape, kw["nof_layers"], seed=11)] * n)
    e_dev = torch.from_numpy(e0.view(np.int32)).to("cuda:0")
    s_dev = torch.zeros((n, grids[0].shape[0], 6), dtype=torch.float32, device="cuda:0")
    est.estimate_batch(g_dev, _config(kw), e_dev, s_dev)
    torch.cuda.synchronize()
    got = e_dev.cpu().numpy().view(np.uint32)
    st = s_dev.cpu().numpy()
    keys = ["noise_var", "epre", "rsrp", "snr", "time_alignment_s", "cfo_hz"]
    for i in range(n):
        want, ws = chest.pusch_chest(grids[i], estimates=e0[i], **kw)
        cc.assert_estimates_close(got[i], want, "grid %d" % i)
        cc.assert_stats_close([dict(zip(keys, row)) for row in st[i]], ws, "grid %d" % i)


STAT_KEYS = ["noise_var", "epre", "rsrp", "snr", "time_alignment_s", "cfo_hz"]


def _check_vs_oracle(got, gs, want, ws, kw, what):
    """The host test's bar: every estimate within two bf16 roundings, the statistics within 2e-3, and at most
    IDENTICAL_CAP of the words different at all -- over the whole buffer and over the allocation's edge band."""
    cc.assert_estimates_close(got, want, what)
    cc.assert_stats_close(gs, ws, what)
    cc.assert_estimates_mostly_identical(got, want, cc.IDENTICAL_CAP, what=what)
    cc.assert_estimates_mostly_identical(got, want, cc.IDENTICAL_CAP, where=cc.edge_band(kw, np.shape(got)),
                                         what=what + " edge band")


def _assert_silent(got_p, st, kw, what):
    """A port that received all-zero words: every measurement exactly 0 (the CFO too: atan2(0, 0), not NaN) and
    every estimate inside the allocation +-0."""
    for k in STAT_KEYS:
        assert float(st[k]) == 0.0, (what, k, st[k])
    sy = slice(kw["first_symbol"], kw["first_symbol"] + kw["nof_symbols"])
    inside = np.asarray(got_p, np.uint32)[:, sy, 12 * kw["prb_lo"]:12 * kw["prb_hi"]]
    assert ((inside & 0x7FFF7FFF) == 0).all(), what


@pytest.mark.parametrize("case", cc.EDGE_CASES, ids=cc.EDGE_IDS)
def test_pusch_chest_coherent_host(est, case):
    """Grids that hold the DM-RS (a known delay, CFO and SNR) at the kernel's edges: every time-alignment IDFT size
    and both workgroup widths, four DM-RS symbols, numerologies 0 / 2 / 3, an advanced UE, a peak at tap 0 and one
    outside the search window, a reported but uncompensated CFO, the SINR ceiling."""
    name = case[0]
    grid, kw, est0, want, ws = cc.edge_args(case)
    got, gs = est.estimate(grid, _config(kw), estimates=est0)
    _check_vs_oracle(got, gs, want, ws, kw, name)
    if oracle.REF is not None:
        want_r, ws_r = chest.ref_pusch_chest(grid, estimates=est0, **kw)
        cc.assert_estimates_close(got, want_r, name + " vs reference")
        cc.assert_stats_close(gs, ws_r, name + " vs reference")
    if case[16] is None:  # no noise: the variance is the floor rsrp / 1e10 (a correctly rounded division), 100 dB
        for p, st in enumerate(gs):
            floor = np.float32(st["rsrp"]) / np.float32(1e10)
            assert np.isclose(float(st["noise_var"]), float(floor), rtol=2.0 ** -22, atol=0), (name, p, st)
            assert abs(10 * np.log10(float(st["snr"])) - 100.0) <= 1e-5, (name, p, st)


# Three ports over 52 PRB, allocation 4..34, two layers, two DM-RS symbols: one grid as received and the same grid
# with port 1 all-zero words.
SILENT_KW = dict(slot_index=3, type2=False, nof_layers=2, scrambling_id=77, n_scid=1, scaling=1.0, symbols_mask=cc.D2,
                 prb_lo=4, prb_hi=34, first_symbol=0, nof_symbols=14, fd=2, td=1, compensate_cfo=True, numerology=1)


@pytest.fixture(scope="module")
def three_ports(est):
    full = cc.coherent_grid(3, 52, SILENT_KW, 15.0, 0.003, 30.0, seed=31)
    silent = cc.coherent_grid(3, 52, SILENT_KW, 15.0, 0.003, 30.0, seed=31, silent=(1,))
    assert np.array_equal(full[[0, 2]], silent[[0, 2]]) and not silent[1].any()
    est0 = cc.stale_estimates(full.shape, 2, seed=7)
    got_full, gs_full = est.estimate(full, _config(SILENT_KW), estimates=est0)
    return full, silent, est0, got_full, gs_full


def test_pusch_chest_silent_port(est, three_ports):
    """A port that receives nothing (atan2f(0, 0), 0 / 0 in the peak refinement, a zero noise variance) reports
    zeros, as the reference does, and leaves the other ports' results untouched."""
    full, silent, est0, got_full, gs_full = three_ports
    got, gs = est.estimate(silent, _config(SILENT_KW), estimates=est0)
    _assert_silent(got[1], gs[1], SILENT_KW, "GPU")
    with np.errstate(all="ignore"):
        want, ws = chest.pusch_chest(silent, estimates=est0, **SILENT_KW)
    _assert_silent(want[1], ws[1], SILENT_KW, "oracle")
    _check_vs_oracle(got, gs, want, ws, SILENT_KW, "silent port")
    if oracle.REF is not None:
        want_r, ws_r = chest.ref_pusch_chest(silent, estimates=est0, **SILENT_KW)
        _assert_silent(want_r[1], ws_r[1], SILENT_KW, "reference")
        cc.assert_estimates_close(got, want_r, "silent port vs reference")
        cc.assert_stats_close(gs, ws_r, "silent port vs reference")
    for p in (0, 2):
        assert np.array_equal(got[p], got_full[p]), p
        assert gs[p] == gs_full[p], (p, gs[p], gs_full[p])


def _word_nan(u):
    z = cc.to_cf(u)
    return np.isnan(z.real) | np.isnan(z.imag)


def test_pusch_chest_nonfinite_contained(est, three_ports):
    """One NaN DM-RS RE on port 0 and one +Inf DM-RS RE on port 2: the call returns, port 1 is untouched, the
    poisoned ports report what the reference does -- SNR 0, NaN noise variance and RSRP -- and NaN estimates wherever
    the reference's are.  (The reference's time alignment of such input is an integer cast of NaN: no contract.)"""
    full, _, est0, got_full, gs_full = three_ports
    grid = full.copy()
    sc = 12 * SILENT_KW["prb_lo"] + 2 * 40  # pilot 40 of CDM group 0
    grid[0, 2, sc] = (grid[0, 2, sc] & 0xFFFF0000) | 0x7FC0  # real part NaN
    grid[2, 11, sc + 2] = (grid[2, 11, sc + 2] & 0xFFFF0000) | 0x7F80  # real part +Inf
    got, gs = est.estimate(grid, _config(SILENT_KW), estimates=est0)
    assert np.array_equal(got[1], got_full[1])
    assert gs[1] == gs_full[1], (gs[1], gs_full[1])
    with np.errstate(all="ignore"):
        if oracle.REF is not None:
            want, ws = chest.ref_pusch_chest(grid, estimates=est0, **SILENT_KW)
        else:
            want, ws = chest.pusch_chest(grid, estimates=est0, **SILENT_KW)
    lo, hi = 12 * SILENT_KW["prb_lo"], 12 * SILENT_KW["prb_hi"]
    for p in (0, 2):
        assert float(ws[p]["snr"]) == 0.0 and np.isnan(ws[p]["noise_var"]) and np.isnan(ws[p]["rsrp"]), (p, ws[p])
        assert float(gs[p]["snr"]) == 0.0, (p, gs[p])
        assert np.isnan(gs[p]["noise_var"]) and np.isnan(gs[p]["rsrp"]), (p, gs[p])
        want_nan = _word_nan(want[p][:, :, lo:hi])
        assert want_nan.any(), p
        assert _word_nan(got[p][:, :, lo:hi])[want_nan].all(), p


def test_pusch_chest_batch_strides(est):
    """The batch form on slices of larger tensors: grid and estimate strides that exceed the tight size by a pad
    that is no multiple of 64 words, a different delay, CFO and stale estimate per grid, the middle grid all-zero.
    Each grid as the host test, the middle one as a silent port, both pads untouched."""
    import torch

    case = cc.EDGE_CASES[cc.EDGE_IDS.index("adv_18prb_N256")]
    kw = cc.edge_kw(case)
    P, nprb, L = case[1], case[2], case[5]
    nsubc = 12 * nprb
    grids = [cc.coherent_grid(P, nprb, kw, -25.5, -0.004, 30.0, seed=41),
             np.zeros((P, 14, nsubc), np.uint32),
             cc.coherent_grid(P, nprb, kw, 33.0, 0.003, 30.0, seed=43)]
    e0 = [cc.stale_estimates(grids[0].shape, L, seed=11 + i) for i in range(3)]
    gsz, esz, gpad, epad = P * 14 * nsubc, P * L * 14 * nsubc, 37, 53
    sentinel = 0x5A5A5A5A
    g_big = torch.full((3, gsz + gpad), sentinel, dtype=torch.int32, device="cuda:0")
    e_big = torch.full((3, esz + epad), sentinel, dtype=torch.int32, device="cuda:0")
    g_dev = g_big[:, :gsz].unflatten(1, (P, 14, nsubc))
    e_dev = e_big[:, :esz].unflatten(1, (P, L, 14, nsubc))
    g_dev.copy_(torch.from_numpy(np.stack(grids).view(np.int32)))
    e_dev.copy_(torch.from_numpy(np.stack(e0).view(np.int32)))
    assert g_dev.stride(0) == gsz + gpad and e_dev.stride(0) == esz + epad
    assert g_dev.data_ptr() == g_big.data_ptr() and e_dev.data_ptr() == e_big.data_ptr()
    s_dev = torch.zeros((3, P, 6), dtype=torch.float32, device="cuda:0")
    est.estimate_batch(g_dev, _config(kw), e_dev, s_dev)
    torch.cuda.synchronize()
    assert (g_big[:, gsz:] == sentinel).all() and (e_big[:, esz:] == sentinel).all()
    assert np.array_equal(g_dev.cpu().numpy().view(np.uint32), np.stack(grids))
    got = e_dev.cpu().numpy().view(np.uint32)
    st = s_dev.cpu().numpy()
    for i in range(3):
        with np.errstate(all="ignore"):
            want, ws = chest.pusch_chest(grids[i], estimates=e0[i], **kw)
        gs = [dict(zip(STAT_KEYS, row)) for row in st[i]]
        _check_vs_oracle(got[i], gs, want, ws, kw, "grid %d" % i)
        if i == 1:
            for p in range(P):
                _assert_silent(got[i][p], gs[p], kw, "grid 1 port %d" % p)


def test_pusch_chest_rejects_unsupported(est):
    import srsran_project_amd as amd

    grid, kw = cc.case_args(cc.CASES[0], seed=1)
    cfg = _config(kw)
    cfg.symbols_mask = 0
    with pytest.raises(ValueError):
        est.estimate(grid, cfg)
    cfg = _config(kw)
    cfg.nof_tx_layers = 5
    with pytest.raises(ValueError):
        est.estimate(grid, cfg)


# Transform precoding: the low-PAPR DM-RS sequence (one layer), against the compiled reference estimator
# configured with low_papr_sequence_configuration (dmrs_pusch_estimator_impl.cpp:86-92).
# (name, ports, nof_prb, rb_start, rb_count, dmrs mask, td, n_rs_id)
LP_CASES = [
    ("lp_1rb_M6", 1, 25, 3, 1, (1 << 2) | (1 << 11), 1, 5),
    ("lp_5rb_M30", 2, 52, 10, 5, (1 << 2) | (1 << 11), 1, 77),
    ("lp_25rb_M150_interp", 4, 52, 20, 25, (1 << 2) | (1 << 7) | (1 << 11), 0, 1007),
    ("lp_270rb_M1620", 2, 273, 2, 270, 1 << 2, 1, 301),
]


@pytest.mark.skipif(oracle.REF is None, reason="oracle/_ref not built")
@pytest.mark.parametrize("case", LP_CASES, ids=[c[0] for c in LP_CASES])
def test_pusch_chest_low_papr_vs_reference(est, case):
    name, P, nprb, lo, cnt, mask, td, n_rs_id = case
    grid = cc.make_grid(P, nprb, 0.05, seed=cnt)
    kw = dict(slot_index=4, type2=2, nof_layers=1, scrambling_id=n_rs_id, n_scid=0, scaling=1.41, symbols_mask=mask,
              prb_lo=lo, prb_hi=lo + cnt, first_symbol=0, nof_symbols=14, fd=2, td=td, compensate_cfo=True,
              numerology=1)
    est0 = cc.stale_estimates(grid.shape, 1, seed=3)
    want, ws = chest.ref_pusch_chest(grid, estimates=est0, **kw)
    cfg = _config(dict(kw, scrambling_id=0))
    cfg.low_papr, cfg.n_rs_id = True, n_rs_id
    got, gs = est.estimate(grid, cfg, estimates=est0)
    cc.assert_estimates_close(got, want, name)
    cc.assert_stats_close(gs, ws, name)


def test_pusch_chest_low_papr_rejects(est):
    grid = cc.make_grid(1, 52, 0.05, seed=0)
    kw = dict(slot_index=0, type2=False, nof_layers=2, scrambling_id=0, n_scid=0, scaling=1.41, symbols_mask=1 << 2,
              prb_lo=0, prb_hi=7, first_symbol=0, nof_symbols=14, fd=2, td=1, compensate_cfo=True, numerology=1)
    cfg = _config(kw)
    cfg.low_papr = True
    with pytest.raises(ValueError):  # two layers
        est.estimate(grid, cfg)
    cfg.nof_tx_layers = 1
    with pytest.raises(ValueError):  # 7 PRB: no low-PAPR sequence of length 42
        est.estimate(grid, cfg)
