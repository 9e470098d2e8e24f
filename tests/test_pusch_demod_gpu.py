"""GPU parity: MI355X PUSCH demodulator (fused RE gather + equalizer, soft
demapper, descrambler; through the C-ABI) against the REFERENCE's own
pusch_demodulator_impl (oracle/_ref, ref_wrapper_pusch.cpp) and the restated
oracle (oracle/pusch_demod.py).

Bars:
  * demapper + descrambler on the reference's own equalized symbols
    (pusch_demod_cases / ref_equalize_per_symbol, the exact values the reference
    class demaps): bit-exact with the reference class, which pins the
    per-OFDM-symbol demapper blocks (pusch_demodulator_impl.cpp:363-400);
  * the same stage on dyadic symbols chosen so that the reference demapper's SIMD
    and scalar-tail arithmetic differ: bit-exact with the reference demapper
    called once per OFDM symbol (and provably different from one call per codeword);
  * full demodulator (GPU float equalizer inside): |dLLR| <= 1 and >= 99 % equal
    against the reference class (>= 97 % on the narrow 16QAM/256QAM cases and the
    identity channels, where the reference's approximate-reciprocal equalizer
    moves more LLRs); codewords of fewer than 1000 LLRs: |dLLR| <= 1 and at most
    max(2, 3 %) of them different.
All of them run over the contiguous type-1 CASES and over MASK_CASES (DM-RS type 2,
CRB masks with holes, allocations of one PRB / one symbol / starting on the DM-RS
symbol, pi/2-BPSK); the plan's data RE count is checked against the restated
selection for every case.
"""
import numpy as np
import pytest

import oracle
from oracle import pusch_demod as od
from tests.pusch_demod_cases import (CASES, MASK_CASES, MIMO_CASES, PINNED_MASK_CASES, SIMD_BLOCK,
                                     UNPINNED_MASK_CASES, assert_case_llrs_close, assert_llrs_close, case_counts,
                                     case_crbs, case_type2, demod_args, dyadic_equalized, make_case)

pytestmark = pytest.mark.gpu

RNTI, N_ID = 0x1234, 321
C_INIT = RNTI * (1 << 15) + N_ID
# t2_cdm3_4x1_256qam: the 7 PRB 256QAM allocation of 2x1_256qam_7prb_tail; holes_2x1_16qam_cdm1: the topology,
# modulation and DM-RS of 2x1_16qam_cdm1 on fewer PRBs
NARROW = {"2x1_16qam_cdm1", "1x1_16qam_5prb_tail", "2x1_256qam_7prb_tail", "t2_cdm3_4x1_256qam",
          "holes_2x1_16qam_cdm1"}
PINNED = CASES + PINNED_MASK_CASES
TIE_CASES = [c for c in CASES + MASK_CASES if c[5] >= 4]


def _cfg(case, crbs):
    import srsran_project_amd as amd

    name, P, L, nprb, _, qm, start, nsym, dmrs, ncdm = case[:10]
    kw = {}
    if len(case) > 10:
        kw["equalizer"] = int(getattr(amd.ChannelEqualizerAlgorithmType, case[10]))
    return amd.PuschDemodulatorConfig(rnti=RNTI, crbs=crbs, modulation=qm, start_symbol=start, nof_symbols=nsym,
                                      dmrs_symb_pos=dmrs, n_id=N_ID, nof_tx_layers=L, nof_rx_ports=P,
                                      nof_cdm_groups_without_data=ncdm, dmrs_type=2 if case_type2(case) else 1, **kw)


def _stats(nv):
    return [{"noise_var": v, "epre": 0, "rsrp": 0, "snr": 0, "time_alignment_s": 0, "cfo_hz": 0} for v in nv]


@pytest.fixture(scope="module")
def dem():
    import srsran_project_amd as amd

    return amd.PuschDemodulator(device=0)


def _gpu_demap(dem, plan, eq, nv):
    import torch

    e = torch.from_numpy(np.ascontiguousarray(eq[None], np.complex64)).to("cuda:0")
    v = torch.from_numpy(np.ascontiguousarray(nv[None], np.float32)).to("cuda:0")
    out = dem.demap_descramble_batch(e, v, plan)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("case", CASES + MASK_CASES, ids=[c[0] for c in CASES + MASK_CASES])
def test_plan_data_re_count(dem, case):
    """The plan's RE table counts the data REs of the restated selection (rb_mask, time allocation, DM-RS type and
    CDM groups without data)."""
    name, P, L, nprb, _, qm, start, nsym, dmrs, ncdm = case[:10]
    crbs = case_crbs(case)
    mask = od.data_re_mask(12 * nprb, crbs, start, nsym, dmrs, case_type2(case), ncdm)
    plan = dem.plan(_cfg(case, crbs), 12 * nprb)
    assert plan.nof_re == int(mask.sum()), name
    assert plan.nof_llrs == int(case_counts(case).sum()) * max(1, qm), name


@pytest.mark.parametrize("case", PINNED, ids=[c[0] for c in PINNED])
def test_demap_descramble_on_reference_equalizer_bit_exact(dem, case):
    grid, est, nv, crbs = make_case(case, 5, "random")
    a = dict(demod_args(case))
    a.pop("qm")
    eq, env = od.ref_equalize_per_symbol(grid, est, nv, crbs, **a)
    want = od.ref_pusch_demodulate(grid, est, nv, RNTI, N_ID, crbs=crbs, **demod_args(case))
    got = _gpu_demap(dem, dem.plan(_cfg(case, crbs), 12 * case[3]), eq, env)
    assert np.array_equal(got, want), "%s: %d LLRs differ from pusch_demodulator_impl" % (case[0],
                                                                                         int((got != want).sum()))


@pytest.mark.parametrize("case", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_demap_blocks_follow_ofdm_symbols(dem, case):
    """Dyadic equalized symbols (many land on the rounding ties where the reference demapper's SIMD and
    scalar paths differ): the GPU equals per-OFDM-symbol demapping exactly."""
    name, P, L, nprb, _, qm, start, nsym, dmrs, ncdm = case[:10]
    crbs = case_crbs(case)
    counts = case_counts(case)
    n = int(counts.sum())
    eq, nv = dyadic_equalized(qm, n, 11, oracle.ref_demodulate)
    want = od.demap_descramble_per_symbol(eq, nv, counts, qm, C_INIT, demod=oracle.ref_demodulate)
    got = _gpu_demap(dem, dem.plan(_cfg(case, crbs), 12 * nprb), eq, nv)
    assert np.array_equal(got, want), "%s: %d LLRs differ" % (name, int((got != want).sum()))
    restated = od.demap_descramble_per_symbol(eq, nv, counts, qm, C_INIT)
    assert np.array_equal(restated, want)
    blk = SIMD_BLOCK[qm]
    if any(c % blk for c in counts):
        whole = od.demap_descramble_per_symbol(eq, nv, [n], qm, C_INIT, demod=oracle.ref_demodulate)
        assert not np.array_equal(whole, want), "case does not exercise a tail"


@pytest.mark.parametrize("case", PINNED, ids=[c[0] for c in PINNED])
@pytest.mark.parametrize("kind", ["random", "identity"])
def test_pusch_demodulate_host_vs_reference(dem, case, kind):
    grid, est, nv, crbs = make_case(case, 3, kind)
    want = od.ref_pusch_demodulate(grid, est, nv, RNTI, N_ID, crbs=crbs, **demod_args(case))
    got = dem.demodulate(grid, est, _stats(nv), _cfg(case, crbs))
    # identity channels: the reference's approximate reciprocal (1 - 2^-12 on |h|^2 = 1) biases every
    # equalized value the same way, so more LLRs sit one step away than on a random channel
    assert_case_llrs_close(case, got, want, case[0], 0.97 if (case[0] in NARROW or kind == "identity") else 0.99)
    # the restated oracle (float64 equalizer) as a second opinion
    rest = od.pusch_demodulate(grid, est, nv, RNTI, N_ID, crbs=crbs, **demod_args(case))
    assert_case_llrs_close(case, got, rest, case[0] + " (restated)", 0.97)


def test_pusch_demodulate_batch(dem):
    import torch

    case = CASES[6]  # 4x2 256QAM 273 PRB
    name, P, L, nprb, _, qm, start, nsym, dmrs, ncdm = case[:10]
    n = 2
    data = [make_case(case, s) for s in range(n)]
    crbs = data[0][3]
    plan = dem.plan(_cfg(case, crbs), 12 * nprb)
    g = torch.from_numpy(np.stack([d[0] for d in data]).view(np.int32)).to("cuda:0")
    e = torch.from_numpy(np.stack([d[1] for d in data]).view(np.int32)).to("cuda:0")
    st = torch.zeros((n, P, 6), dtype=torch.float32)
    for i in range(n):
        st[i, :, 0] = torch.from_numpy(data[i][2])
    llrs = dem.demodulate_batch(g, e, st.to("cuda:0"), plan)
    torch.cuda.synchronize()
    got = llrs.cpu().numpy()
    for i in range(n):
        want = od.ref_pusch_demodulate(data[i][0], data[i][1], data[i][2], RNTI, N_ID, crbs=crbs,
                                       **demod_args(case))
        assert_llrs_close(got[i], want, "grid %d" % i)


def test_pusch_demodulate_batch_holes_sentinel(dem):
    """Three grids of the holed type-2 allocation through the device form, LLR rows 64 bytes longer than the
    codeword rounded up to 64 and pre-filled: every row equals the host form and nothing at or beyond the codeword
    length is written."""
    import torch

    case = next(c for c in MASK_CASES if c[0] == "holes_t2_4x2_256qam")
    name, P, L, nprb = case[:4]
    n = 3
    data = [make_case(case, 20 + s) for s in range(n)]
    crbs = data[0][3]
    plan = dem.plan(_cfg(case, crbs), 12 * nprb)
    G = plan.nof_llrs
    assert G == int(case_counts(case).sum()) * case[5]
    g = torch.from_numpy(np.stack([d[0] for d in data]).view(np.int32)).to("cuda:0")
    e = torch.from_numpy(np.stack([d[1] for d in data]).view(np.int32)).to("cuda:0")
    st = torch.zeros((n, P, 6), dtype=torch.float32)
    for i in range(n):
        st[i, :, 0] = torch.from_numpy(data[i][2])
    llrs = torch.full((n, (G + 63) // 64 * 64 + 64), -77, dtype=torch.int8, device="cuda:0")
    dem.demodulate_batch(g, e, st.to("cuda:0"), plan, llrs=llrs)
    torch.cuda.synchronize()
    got = llrs.cpu().numpy()
    assert (got[:, G:] == -77).all(), "bytes beyond the codeword written"
    for i in range(n):
        host = dem.demodulate(data[i][0], data[i][1], _stats(data[i][2]), plan)
        assert np.array_equal(got[i, :G], host), "grid %d" % i
    assert not np.array_equal(got[0, :G], got[1, :G])


UNPINNED = MIMO_CASES + UNPINNED_MASK_CASES


@pytest.mark.parametrize("case", UNPINNED, ids=[c[0] for c in UNPINNED])
def test_pusch_demodulate_mimo_unpinned(dem, case):
    """3 and 4 layers (ZF / MMSE) and 2-layer MMSE: the open reference's equalizer asserts for these topologies,
    so the demodulator is checked against the restated chain with the fp64 L-layer solve (PARITY UNPINNED for the
    equalizer; RE selection, demapper blocks and descrambling are the pinned ones): |dLLR| <= 1, >= 99 % equal."""
    grid, est, nv, crbs = make_case(case, 11, "mimo")
    got = dem.demodulate(grid, est, _stats(nv), _cfg(case, crbs))
    want = od.pusch_demodulate(grid, est, nv, RNTI, N_ID, crbs=crbs, **demod_args(case))
    assert_llrs_close(got, want, case[0], 0.99)
