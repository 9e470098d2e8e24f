"""Shared PUSCH channel-estimation test cases: synthetic received grids
(a frequency-selective, slowly rotating channel times random QPSK-like data
plus noise, the shapes of the reference's dmrs_pusch_estimator vector tests:
tests/unittests/phy/upper/signal_processors/dmrs_pusch_estimator_test_data.h,
whose .dat files are not in the reference tree) and the estimator settings."""
import numpy as np

from oracle.pdsch_mod import to_bf16

# (name, ports, nof_prb, rb_start, rb_count, layers, dmrs mask, first, nsym, fd, td, cfo, scaling, noise)
CASES = [
    ("1x1_52prb_filter_avg", 1, 52, 0, 52, 1, (1 << 2) | (1 << 11), 0, 14, 2, 1, True, 1.0, 0.05),
    ("2x2_part_filter_avg", 2, 52, 4, 36, 2, (1 << 2) | (1 << 11), 0, 14, 2, 1, True, 1.0, 0.05),
    ("4x4_273prb_filter_avg", 4, 273, 0, 273, 4, (1 << 2) | (1 << 11), 0, 14, 2, 1, True, 1.0, 0.02),
    ("2x4_interp", 2, 52, 0, 52, 4, (1 << 2) | (1 << 7) | (1 << 11), 0, 14, 2, 0, True, 1.0, 0.05),
    ("1rb", 1, 25, 3, 1, 1, 1 << 2, 0, 14, 2, 1, True, 1.0, 0.05),
    ("mean_nocfo_1dmrs", 2, 52, 0, 52, 2, 1 << 3, 1, 13, 1, 1, False, 1.0, 0.05),
    ("none_interp_4rx", 4, 106, 10, 90, 2, (1 << 2) | (1 << 7) | (1 << 11), 0, 14, 0, 0, True, 1.0, 0.05),
    ("3layers_interp", 2, 52, 0, 52, 3, (1 << 2) | (1 << 3), 0, 14, 2, 0, True, 1.0, 0.05),
    ("scaled_2rb", 1, 24, 5, 2, 1, (1 << 2) | (1 << 9), 2, 10, 2, 1, True, 1.41, 0.1),
]


D2 = (1 << 2) | (1 << 11)
D3 = (1 << 2) | (1 << 7) | (1 << 11)
D4 = (1 << 2) | (1 << 5) | (1 << 8) | (1 << 11)

# Coherent grids (coherent_grid: the real DM-RS through a smooth channel with a known delay and CFO) at the
# estimator's edges: both sides of every time-alignment IDFT size (17/18, 34/35, 68/69 -- also the narrow / wide
# workgroups --, 137/138 PRB) and the 275-PRB maximum, four DM-RS symbols, numerologies 0, 2 and 3, an advanced
# UE, a peak at tap 0 and one outside the half-CP window, both CFO signs, a CFO that is reported but not
# compensated, one DM-RS symbol with 3 / 4 layers, the 15-tap filter (3 PRB) and the SINR ceiling (no noise).
# delay in units of 1 / (4096 scs), cfo in cycles per symbol duration, snr None: no noise.
# (name, ports, nof_prb, rb_start, rb_count, layers, dmrs mask, first, nsym, fd, td, compensate_cfo, numerology,
#  slot, delay, cfo, snr dB, scaling)
EDGE_CASES = [
    ("adv_17prb_N128", 2, 25, 5, 17, 1, D2, 0, 14, 2, 1, True, 1, 3, -40.0, 0.004, 30.0, 1.0),
    ("adv_18prb_N256", 2, 25, 5, 18, 2, D2, 0, 14, 2, 1, True, 1, 3, -25.5, -0.004, 30.0, 1.0),
    ("zero_ta_34prb_N256_mu0", 1, 52, 7, 34, 2, D2, 0, 14, 2, 1, True, 0, 5, 0.0, 0.0, 40.0, 1.0),
    ("35prb_N512_mu0_3l", 2, 52, 7, 35, 3, D2, 0, 14, 2, 1, True, 0, 9, 60.0, 0.002, 25.0, 1.41),
    ("68prb_narrow", 2, 106, 11, 68, 4, D2, 0, 14, 2, 1, True, 1, 4, -90.3, 0.003, 30.0, 1.0),
    ("69prb_wide", 2, 106, 11, 69, 4, D2, 0, 14, 2, 1, True, 1, 4, -90.3, 0.003, 30.0, 1.0),
    ("137prb_N1024", 1, 273, 3, 137, 2, D2, 0, 14, 2, 1, True, 1, 7, 120.0, -0.003, 30.0, 1.0),
    ("138prb_N2048", 1, 273, 3, 138, 2, D2, 0, 14, 2, 1, True, 1, 7, -120.0, -0.003, 30.0, 1.0),
    ("275prb_max", 1, 275, 0, 275, 4, D2, 0, 14, 2, 1, True, 1, 19, 100.0, 0.002, 35.0, 1.0),
    ("4dmrs_avg_4l", 2, 52, 1, 21, 4, D4, 0, 14, 2, 1, True, 1, 2, 30.0, 0.003, 30.0, 1.0),
    ("4dmrs_interp_3l", 2, 52, 1, 21, 3, D4, 0, 14, 2, 0, True, 1, 2, -30.0, -0.003, 30.0, 1.0),
    ("nocomp_2dmrs", 2, 52, 0, 20, 2, D2, 0, 14, 2, 1, False, 1, 3, 10.0, 0.004, 30.0, 1.0),
    ("1dmrs_3l_interp", 2, 52, 0, 20, 3, 1 << 3, 1, 13, 2, 0, True, 1, 3, 10.0, 0.0, 30.0, 1.0),
    ("1dmrs_4l_mean", 2, 52, 0, 20, 4, 1 << 3, 1, 13, 1, 1, True, 1, 3, 10.0, 0.0, 30.0, 1.0),
    ("3prb_15taps", 2, 24, 20, 3, 2, D2, 0, 14, 2, 1, True, 1, 3, 5.0, 0.002, 30.0, 1.0),
    ("mu2_slot1_interp", 2, 52, 2, 24, 2, D3, 0, 14, 2, 0, True, 2, 1, -20.0, 0.003, 30.0, 1.0),
    ("mu3_slot5_none", 1, 66, 0, 66, 1, D2, 0, 14, 0, 1, True, 3, 5, 40.0, -0.003, 30.0, 1.0),
    ("hi_snr_50", 2, 52, 0, 52, 2, D2, 0, 14, 2, 1, True, 1, 3, 12.0, 0.001, 50.0, 1.0),
    ("ta_beyond_window", 1, 52, 0, 52, 1, D2, 0, 14, 2, 1, True, 1, 3, 200.0, 0.0, 30.0, 1.0),
    ("sinr_ceiling_1dmrs", 1, 25, 2, 10, 1, 1 << 2, 0, 14, 0, 1, True, 1, 3, 0.0, 0.0, None, 1.0),
    ("sinr_ceiling_2dmrs", 1, 25, 2, 10, 1, D2, 0, 14, 0, 1, True, 1, 3, 0.0, 0.0, None, 1.0),
]
EDGE_IDS = [c[0] for c in EDGE_CASES]
# share of estimate words that may differ at all from the oracle's: a float32 disagreement of k ulps flips a bf16
# rounding with probability k 2^-16; a word has two components and up to two roundings (the estimate, then its
# CFO rotation), so the share is 4 k 2^-16 -- 1e-3 at k = 16 ulps of reassociated sums
IDENTICAL_CAP = 1e-3
EDGE_BAND = 24  # REs at either end of the allocation where the virtual pilots and the truncated FIR window act


def bf16_grid(c):
    return (to_bf16(c.real.astype(np.float32)).astype(np.uint32)
            | (to_bf16(c.imag.astype(np.float32)).astype(np.uint32) << 16))


def make_grid(ports, nof_prb, noise, seed):
    rng = np.random.default_rng(seed)
    nsubc = 12 * nof_prb
    k = np.arange(nsubc)
    g = np.zeros((ports, 14, nsubc), np.complex64)
    for p in range(ports):
        h = (0.8 + 0.3j) * np.exp(-2j * np.pi * k * (3 + p) / 4096) * (1 + 0.2 * np.cos(k / 200 + p))
        for l in range(14):
            d = (rng.choice([-1, 1], nsubc) + 1j * rng.choice([-1, 1], nsubc)) * 0.7
            g[p, l] = h * np.exp(1j * 0.01 * l) * d + noise * (rng.normal(size=nsubc) + 1j * rng.normal(size=nsubc))
    return bf16_grid(g)


def case_args(case, seed=0):
    name, P, nprb, lo, cnt, L, mask, first, ns, fd, td, cfo, scaling, noise = case
    grid = make_grid(P, nprb, noise, seed)
    kw = dict(slot_index=3 + seed, type2=False, nof_layers=L, scrambling_id=77 + seed, n_scid=seed % 2,
              scaling=scaling, symbols_mask=mask, prb_lo=lo, prb_hi=lo + cnt, first_symbol=first, nof_symbols=ns,
              fd=fd, td=td, compensate_cfo=cfo, numerology=1)
    return grid, kw


def coherent_grid(P, nof_prb, kw, delay, cfo, snr_db, seed, silent=(), numerology=1):
    """A received grid that holds the DM-RS the estimator looks for.  Layer v reaches port p through
    h[p, v][k] = c[p, v] (1 + 0.2 cos(k / 200 + p + v)) exp(-2j pi k (delay + 0.25 p) / 4096): a distinct phase per
    (port, layer), a mild ripple and a linear phase, delay in units of 1 / (4096 scs) (negative: an advanced
    UE).  DM-RS symbols carry sum_v h[p, v] pil[v] scaling on the pilots' subcarriers, the other symbols random
    QPSK through the same channel; symbol l turns by exp(2j pi cfo epoch[l]) (cfo in cycles per symbol duration);
    AWGN at snr_db below the mean RE power (None: no noise); the ports in `silent` are all-zero words."""
    from oracle import chest

    rng = np.random.default_rng(seed)
    nsubc = 12 * nof_prb
    L, lo, hi = kw["nof_layers"], kw["prb_lo"], kw["prb_hi"]
    pil, syms = chest.pilots(kw["slot_index"], False, L, kw["scrambling_id"], kw["n_scid"], kw["symbols_mask"], lo, hi)
    k = np.arange(nsubc)
    h = np.zeros((P, L, nsubc), np.complex128)
    for p in range(P):
        for v in range(L):
            h[p, v] = (0.8 * np.exp(1j * (0.4 + 0.9 * p + 1.7 * v)) * (1 + 0.2 * np.cos(k / 200 + p + v))
                       * np.exp(-2j * np.pi * k * (delay + 0.25 * p) / 4096))
    z = np.zeros((P, 14, nsubc), np.complex128)
    for l in range(14):
        d = (rng.choice([-1, 1], (L, nsubc)) + 1j * rng.choice([-1, 1], (L, nsubc))) * np.sqrt(0.5 / L)
        z[:, l] = np.einsum("pvk,vk->pk", h, d)
    m = np.arange(pil.shape[2])
    for d, l in enumerate(syms):
        z[:, l, 12 * lo:12 * hi] = 0
        for v in range(L):
            sc = 12 * lo + 2 * m + v // 2
            z[:, l, sc] += h[:, v, sc] * pil[v, d][None, :] * kw["scaling"]
    epoch = chest.symbol_start_epochs(numerology).astype(np.float64)
    z *= np.exp(2j * np.pi * cfo * epoch)[None, :, None]
    if snr_db is not None:
        sigma = np.sqrt(float(np.mean(np.abs(z[np.abs(z) > 0]) ** 2)) / 10 ** (snr_db / 10) / 2)
        z += sigma * (rng.normal(size=z.shape) + 1j * rng.normal(size=z.shape))
    for p in silent:
        z[p] = 0
    return bf16_grid(z)


def edge_kw(case):
    name, P, nprb, lo, cnt, L, mask, first, ns, fd, td, ccfo, mu, slot, delay, cfo, snr, scaling = case
    return dict(slot_index=slot, type2=False, nof_layers=L, scrambling_id=77, n_scid=slot % 2, scaling=scaling,
                symbols_mask=mask, prb_lo=lo, prb_hi=lo + cnt, first_symbol=first, nof_symbols=ns, fd=fd, td=td,
                compensate_cfo=ccfo, numerology=mu)


_edge_cache = {}


def edge_args(case):
    """(grid, settings, stale estimates, oracle estimates, oracle statistics) of an EDGE_CASES row, computed once
    per process and shared by the tests that need them (none of them writes to these arrays)."""
    from oracle import chest

    name, P, nprb, lo, cnt, L, mask, first, ns, fd, td, ccfo, mu, slot, delay, cfo, snr, scaling = case
    if name not in _edge_cache:
        kw = edge_kw(case)
        grid = coherent_grid(P, nprb, kw, delay, cfo, snr, seed=100 + EDGE_IDS.index(name), numerology=mu)
        est0 = stale_estimates(grid.shape, L, seed=7)
        with np.errstate(all="ignore"):
            want, ws = chest.pusch_chest(grid, estimates=est0, **kw)
        for a in (grid, est0, want):
            a.setflags(write=False)
        _edge_cache[name] = (grid, kw, est0, want, ws)
    return _edge_cache[name]


def edge_truth(case):
    """What an EDGE_CASES row injects, in the units of the statistics: the delay in seconds, one tap of the
    time-alignment IDFT (N = max(128, pow2ceil(npil 4096 / 3300)) points over the pilots, two subcarriers apart),
    half a cyclic prefix (the search window) and the CFO in Hz."""
    cnt, mu, delay, cfo = case[4], case[12], case[14], case[15]
    scs = (15 << mu) * 1000.0
    n = max(128, 1 << int(np.ceil(np.log2(max(6 * cnt * 4096 // 3300, 1)))))
    return dict(ta_s=delay / (4096 * scs), tap_s=1 / (n * scs * 2), half_cp_s=144 * 64 / (1 << (mu + 1)) / (480e3 * 4096),
                cfo_hz=cfo * scs, ta_n=n)


def edge_band(kw, shape):
    """Mask [ports][layers][14][nsubc] of the first and last EDGE_BAND REs of the allocation in every written
    symbol."""
    band = np.zeros(shape, bool)
    lo, hi = 12 * kw["prb_lo"], 12 * kw["prb_hi"]
    sy = slice(kw["first_symbol"], kw["first_symbol"] + kw["nof_symbols"])
    band[:, :, sy, lo:min(lo + EDGE_BAND, hi)] = True
    band[:, :, sy, max(hi - EDGE_BAND, lo):hi] = True
    return band


def share_differing(got, want, where=None):
    """(number of estimate words that are not bit-identical, number of words looked at)."""
    diff = np.asarray(got, np.uint32) != np.asarray(want, np.uint32)
    if where is not None:
        diff = diff[where]
    return int(diff.sum()), int(diff.size)


def assert_estimates_mostly_identical(got, want, cap, where=None, what=""):
    """At most `cap` of the estimate words differ at all (over the words of the mask `where`: at most
    max(2, cap n)).  The companion of assert_estimates_close, which bounds how far a word may be off but not how
    many are: a bias below its 2^-6 bar moves most roundings."""
    bad, n = share_differing(got, want, where)
    allowed = cap * n if where is None else max(2, cap * n)
    assert bad <= allowed, "%s: %d of %d estimate words differ (share %.2e, cap %.1e)" % (what, bad, n, bad / n, cap)


def stale_estimates(grid_shape, nof_layers, seed=2):
    """Finite stale contents of an estimate buffer (the reference rotates them by the CFO phase)."""
    rng = np.random.default_rng(seed)
    shape = (grid_shape[0], nof_layers) + tuple(grid_shape[1:])
    return bf16_grid((rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64))


def to_cf(u):
    u = np.asarray(u, np.uint32)
    return ((u & 0xFFFF) << 16).view(np.float32) + 1j * ((u >> 16) << 16).view(np.float32)


def assert_estimates_close(got, want, what=""):
    """bf16 estimates: equal up to the two bf16 roundings of a float-reassociated value (the estimate, then
    the CFO-rotated estimate): 2^-6 relative of the larger magnitude of the pair, plus 1e-6 absolute."""
    same = np.asarray(got, np.uint32) == np.asarray(want, np.uint32)
    a, b = to_cf(got), to_cf(want)
    with np.errstate(invalid="ignore", over="ignore"):
        tol = 2.0 ** -6 * np.maximum(np.abs(a), np.abs(b)) + 1e-6
        bad = ~same & ~(np.abs(a - b) <= tol)
    assert not bad.any(), "%s: %d of %d estimates differ (max %.3e)" % (what, bad.sum(), bad.size,
                                                                       np.abs(a - b)[bad].max())


def assert_stats_close(got, want, what=""):
    for p, (x, y) in enumerate(zip(got, want)):
        for k in ("noise_var", "epre", "rsrp", "snr"):
            assert np.isclose(float(x[k]), float(y[k]), rtol=2e-3, atol=1e-12), (what, p, k, x[k], y[k])
        tx, ty = float(x["time_alignment_s"]), float(y["time_alignment_s"])
        assert abs(tx - ty) <= 2e-3 * abs(ty) + 2e-9, (what, p, "ta", tx, ty)
        cx, cy = float(x["cfo_hz"]), float(y["cfo_hz"])
        assert (np.isnan(cx) and np.isnan(cy)) or np.isclose(cx, cy, rtol=2e-3, atol=1e-2), (what, p, "cfo", cx, cy)
