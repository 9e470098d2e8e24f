"""GPU: the 64QAM / 256QAM soft demapper at its interval edges, and the equalizer kernels' descrambling demapper.

Expected LLRs come from the compiled reference demapper (oracle.ref_demodulate; the restated oracle.demodulate
where oracle/_ref is not built), never from the library under test.

Stand-alone demapper (Modulator.demodulate_soft): every special component value below visits every position of
calls of 1, 7, 8, 9, 15, 16, 17 and 40 symbols (SIMD blocks of 16 symbols for 64QAM and 4 for 256QAM, the scalar
tail, and the border between them), real and imaginary part taking different values, the noise variances cycling
through a small and a large normal value, one near FLT_MIN, 1e20, 0 and -1.  The values: every interval edge
j 2a from two intervals below the constellation to two above it, each also one ulp up and down; 0, -0, +-1e-9 and
its neighbours, 1e-30, a subnormal; magnitudes on both sides of 2^31, 2^32 and 2^33 fine interval widths (where
x / width leaves the int32 range for the fine tables and for the twice as wide LSB table), +-3e38; NaN and
+-infinity.  The compiled reference returns the same LLRs for a NaN or infinite component at every position of a
SIMD block and of a scalar-only call (checked on the CPU, both parts, noise variances 0.01 and 50), so the
non-finite values have one expectation and take part.

What these inputs found: with the line computed as a product rounded before the sum (as the library did before
this test), the ten (qm, n) with a SIMD block fail -- 164 (64QAM) and 604 (256QAM) LLRs, every one a SIMD-block
symbol with the noise variance 1.2e-38 and a component on a zero crossing of its line (for instance x = -3 * 2a
in the 64QAM LSB table): 0 where the compiled reference has -120 or +120.  avx2_helpers.h writes _mm256_mul_ps,
then _mm256_add_ps, and the x86-64-v3 build of the reference contracts the pair into one fused multiply-add, which
keeps a residue of the order of 1e-8 that the reciprocal 8.3e37 saturates.  demap_device.h now writes that fused
multiply-add out, as it already did for the scalar tail.

Equalizer kernels (PuschDemodulator: pusch_equalize_kernel, whose equalize_write / emit_llrs the estimator-fused
pusch_equalize_fused_kernel shares; tests/test_pusch_fused_topologies_gpu.py holds the two bit-identical at
every instantiation): 1 and 3 PRB, two data symbols around a DM-RS symbol, every topology the kernels
instantiate, 64QAM and 256QAM, three (rnti, n_id) pairs, an identity channel whose grid samples put interval
edges, zeros and tiny values among random ones.  The reference's equalizer multiplies by an approximate
reciprocal, so the reference demodulator's LLRs are within one step of the GPU's but not equal to them
(tests/test_pusch_demod_gpu.py), and it has no four-layer or MMSE equalizer: the LLR rows are compared for
equality with the reference demapper (one call per OFDM symbol) and the restated descrambler applied to the
equalized symbols and noise variances of the library's stand-alone ChannelEqualizer, which runs the same
device functions on the same REs.
"""
import numpy as np
import pytest

import oracle
from oracle import pusch_demod as od
from tests.chest_cases import bf16_grid

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 9, 15, 16, 17, 40]
NOISE_VARS = np.array([1e-3, 50.0, 1.2e-38, 1e20, 0.0, -1.0], np.float32)
if oracle.REF is None:
    # On an interval edge the line's value is a rounding residue that a reciprocal of 1e37 and more turns into a
    # saturated LLR.  The compiled reference and the GPU have that residue, the restated oracle computes an exact 0
    # (they agree on all the other values here, checked on the CPU): without the reference, no such variance.
    NOISE_VARS = np.delete(NOISE_VARS, 2)
PAM_A = {6: np.float32(1.0) / np.sqrt(np.float32(42.0)), 8: np.float32(1.0) / np.sqrt(np.float32(170.0))}


def _ref_demod(s, nv, qm):
    return (oracle.ref_demodulate if oracle.REF is not None else oracle.demodulate)(s, nv, qm)


def _around(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def special_values(qm, non_finite=True):
    w = np.float32(2.0) * PAM_A[qm]  # fine interval width
    half = (1 << (qm // 2)) // 2     # intervals on each side of zero
    vals = []
    for j in range(-(half + 2), half + 3):
        vals += _around(np.float32(j) * w)
    vals += [np.float32(0.0), np.float32(-0.0), np.float32(1e-30), np.float32(1e-40)]
    vals += _around(1e-9) + _around(-1e-9)
    for t in (2.0 ** 31, 2.0 ** 32, 2.0 ** 33):
        vals += _around(np.float32(t) * w) + _around(-np.float32(t) * w)
    vals += [np.float32(3e38), np.float32(-3e38)]
    if non_finite:
        vals += [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    return np.array(vals, np.float32)


@pytest.fixture(scope="module")
def mod():
    import srsran_project_amd as amd

    return amd.Modulator()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("qm", [6, 8])
def test_demodulate_soft_interval_edges(mod, qm, n):
    vals = special_values(qm)
    N = vals.size
    i = np.arange(n)
    seen = np.zeros((N, n), bool)
    bad = []
    with np.errstate(all="ignore"):
        for o in range(N):
            re = (o + i) % N
            im = (o + i + 37) % N
            s = np.empty(n, np.complex64)
            s.real, s.imag = vals[re], vals[im]  # (x + 1j * inf would make the real part NaN)
            nv = NOISE_VARS[(o + 2 * i) % NOISE_VARS.size]
            seen[re, i] = True
            got = mod.demodulate_soft(s, nv, qm)
            want = _ref_demod(s, nv, qm)
            if not np.array_equal(got, want):
                k = int(np.nonzero(got != want)[0][0])
                bad.append((o, k // qm, k % qm, s[k // qm], nv[k // qm], int(got[k]), int(want[k])))
    assert seen.all(), "a special value missed a position"
    assert not bad, "%d of %d calls differ; first (call, symbol, bit, value, noise var, got, want): %s" % (
        len(bad), N, bad[:4])


# --- the equalizer kernels' demapper: descrambling inside the quantizer, LLR bytes packed in registers -----------

TOPOLOGIES = [(1, 1, "zf"), (2, 1, "zf"), (4, 1, "zf"), (2, 2, "zf"), (4, 2, "zf"), (4, 3, "zf"), (4, 4, "zf"),
              (2, 2, "mmse"), (4, 2, "mmse"), (4, 3, "mmse"), (4, 4, "mmse")]
SCRAMBLING = [(0x1234, 321), (0xFFFF, 1023), (1, 0)]
EQ_CASES = [(P, L, alg, qm, nprb) for (P, L, alg) in TOPOLOGIES for qm in (6, 8) for nprb in (1, 3)]
NPRB, START, NSYM, DMRS = 4, 1, 3, 1 << 2


def _planted(qm, rng, shape):
    """Transmitted components: half random, half from the interval edges (as bf16 and its neighbours), zeros and
    tiny values."""
    w = np.float32(2.0) * PAM_A[qm]
    half = (1 << (qm // 2)) // 2
    pool = []
    for j in range(-(half + 1), half + 2):
        e = (np.float32(j) * w).view(np.uint32) & np.uint32(0xFFFF0000)
        pool += [np.uint32(e).view(np.float32), np.uint32(e + 0x10000).view(np.float32)]
    pool += [0.0, -0.0, 1e-9, -1e-9, 1e-30, 2e-9, 1e4, -1e4]
    pool = np.array(pool, np.float32)
    x = rng.uniform(-1.3, 1.3, shape).astype(np.float32)
    pick = rng.random(shape) < 0.5
    x[pick] = pool[rng.integers(0, pool.size, int(pick.sum()))]
    return x


@pytest.fixture(scope="module")
def dem():
    import srsran_project_amd as amd

    return amd.PuschDemodulator(device=0)


@pytest.mark.parametrize("idx", range(len(EQ_CASES)), ids=["%dx%d_%s_qm%d_%dprb" % c for c in EQ_CASES])
def test_equalizer_demapper_llrs_equal_reference_demapper(dem, idx):
    import srsran_project_amd as amd

    P, L, alg, qm, nprb = EQ_CASES[idx]
    rnti, n_id = SCRAMBLING[idx % len(SCRAMBLING)]
    crbs = [2] if nprb == 1 else [1, 2, 3]
    ncdm = 1 if L <= 2 else 2
    nsubc = 12 * NPRB
    rng = np.random.default_rng(400 + idx)
    h = np.zeros((P, L, 14, nsubc), np.complex64)
    for p in range(P):
        h[p, p % L] = 1.0
    x = _planted(qm, rng, (L, 14, nsubc)) + 1j * _planted(qm, rng, (L, 14, nsubc))
    grid, est = bf16_grid(np.einsum("pvls,vls->pls", h, x)), bf16_grid(h)
    nv = np.full(P, 2.0 ** -4, np.float32)
    algorithm = getattr(amd.ChannelEqualizerAlgorithmType, alg)
    cfg = amd.PuschDemodulatorConfig(rnti=rnti, crbs=crbs, modulation=qm, start_symbol=START, nof_symbols=NSYM,
                                     dmrs_symb_pos=DMRS, n_id=n_id, nof_tx_layers=L, nof_rx_ports=P,
                                     nof_cdm_groups_without_data=ncdm, dmrs_type=1, equalizer=int(algorithm))
    stats = [{"noise_var": v, "epre": 0, "rsrp": 0, "snr": 0, "time_alignment_s": 0, "cfo_hz": 0} for v in nv]
    got = dem.demodulate(grid, est, stats, cfg)

    mask = od.data_re_mask(nsubc, crbs, START, NSYM, DMRS, False, ncdm)
    ls, ks = np.nonzero(mask)
    sym = np.ascontiguousarray(grid[:, ls, ks]).view(np.uint16)
    he = np.ascontiguousarray(np.transpose(est[:, :, ls, ks], (1, 0, 2))).view(np.uint16)
    eq, env = amd.ChannelEqualizer(algorithm, device=0).equalize(sym, he, nv)
    counts = mask.sum(axis=1) * L
    want = od.demap_descramble_per_symbol(eq.reshape(-1), env.reshape(-1), counts, qm, rnti * (1 << 15) + n_id,
                                          demod=_ref_demod)
    assert got.shape == want.shape
    assert np.abs(want.astype(np.int16)).max() > 0, "every expected LLR is zero"
    assert np.array_equal(got, want), "%d of %d LLRs differ" % (int((got != want).sum()), got.size)
