"""The strong-input LDPC cases against the oracle alone (no GPU).

tests/test_ldpc_decoder_gpu.py compares the kernels with the oracle bit for bit on these inputs; that only proves
something where the inputs reach the code in question.  For every input set those tests use, this file checks that
the CRC early stop both fires after the first iteration and fails, that the LLRs are saturated (beyond the +-64 clamp
of full nodes, up to +-127), that every partial tail node holds a value the clamp would change, and that infinite
soft bits reach the export.
"""
import numpy as np
import pytest

import oracle
from tests import ldpc_cases
from tests.ldpc_cases import strong_codeblocks, force_tail_extremes, strong_inputs

CASES = ldpc_cases.all_cases()


def _id(case):
    return "bg%d-Z%d-L%d..%d-crc%d-F%d%s-s%d" % (case.bg, case.Z, min(case.lens), max(case.lens), case.crc,
                                                case.filler, "r" if case.random_fillers else "", case.seed)


def test_strong_codeblocks_values_and_layout():
    bg, Z, F, crc = 2, 36, 5, 3
    K, N = 10 * Z, 50 * Z
    msgs, llrs = strong_codeblocks(bg, Z, 6, seed=4, crc_poly=crc, filler=F)
    assert msgs.shape == (6, K) and llrs.shape == (6, N) and llrs.dtype == np.int8
    mag = np.abs(llrs.astype(np.int32))
    assert ((mag <= 120) | (mag == 127)).all() and (llrs != -128).all()
    assert (mag == 127).any() and (mag == 120).any()
    for i in range(6):
        assert (msgs[i, K - F:] == 0).all()
        assert oracle.crc_bits(crc, msgs[i, :K - F]) == 0  # information bits followed by their CRC
        assert (llrs[i, K - 2 * Z - F:K - 2 * Z] == 127).all()
    # seeded
    np.testing.assert_array_equal(llrs, strong_codeblocks(bg, Z, 6, seed=4, crc_poly=crc, filler=F)[1])
    # a noiseless row is the codeword
    _, clean = strong_codeblocks(bg, Z, 1, seed=4, noises=(0,), crc_poly=crc, filler=F)
    cw = oracle.ldpc_encode(msgs[0], bg, Z)
    np.testing.assert_array_equal(clean[0] < 0, cw == 1)
    # message bits in the filler positions: the CRC still ends before them, no +127
    msgs, llrs = strong_codeblocks(bg, Z, 6, seed=4, crc_poly=crc, filler=F, random_fillers=True)
    assert msgs[:, K - F:].any() and (np.abs(llrs[:, K - 2 * Z - F:K - 2 * Z].astype(np.int32)) <= 127).all()
    assert all(oracle.crc_bits(crc, msgs[i, :K - F]) == 0 for i in range(6))


def test_force_tail_extremes():
    Z = 8
    llrs = np.tile(np.array([3, -3], np.int8), (4, 20))
    lens = [40, 33, 39, 18]
    before = llrs.copy()
    force_tail_extremes(llrs, lens, Z)
    np.testing.assert_array_equal(llrs[0], before[0])  # whole nodes: untouched
    assert llrs[1, 32] == 127 and (llrs[1, :32] == before[1, :32]).all()  # one-LLR tail
    assert llrs[2, 32] == 127 and llrs[2, 38] == 120
    assert llrs[3, 16] == 127 and llrs[3, 17] == -120
    changed = llrs != before
    assert changed.sum() == 5


def test_case_lengths_cover_the_edges():
    for bg, Z in ldpc_cases.RAGGED_BZ:
        Ls = ldpc_cases.unaligned_lengths(bg, Z)
        assert sorted(L % 4 for L in Ls) == [1, 2, 3]
        assert {1, Z - 1} <= {L % Z for L in Ls}
        rag = ldpc_cases.ragged_lengths(bg, Z)
        assert {L % Z for L in rag} >= {0, 1, 2, Z - 1}
        assert all(ldpc_cases.min_length(bg, Z) <= L <= ldpc_cases.full_length(bg, Z) for L in Ls + rag)
    assert {(-c[4]) % 4 for c in ldpc_cases.FILLER_CASES} == {1, 2, 3}  # filler / CRC boundary inside a word


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_strong_case_is_not_vacuous(case):
    _, llrs = strong_inputs(case)
    K = oracle.BG_K[case.bg] * case.Z
    its, soft_inf, filler_ones = [], False, False
    for i, L in enumerate(case.lens):
        row = llrs[i, :L]
        mag = np.abs(row.astype(np.int32))
        assert ((mag <= 120) | (mag == 127)).all()
        assert (mag > 64).mean() >= 0.05, (i, (mag > 64).mean())
        assert (mag == 127).any()
        if L % case.Z:
            assert (mag[(L // case.Z) * case.Z:] > 64).any(), i
        r, bits, soft = oracle.ldpc_decode(row, case.bg, case.Z, case.iters, "simd", case.crc, case.filler,
                                           ldpc_cases.crc_len(case.crc), force_decoding=bool(case.short),
                                           want_soft=True)
        its.append(r)
        soft_inf = soft_inf or bool((np.abs(soft.astype(np.int32)) == 127).any())
        if r is not None and case.filler:
            filler_ones = filler_ones or bool(oracle.unpack_bits(bits, K)[K - case.filler:].any())
    assert any(r is not None and r >= 2 for r in its), its
    assert any(r is None for r in its), its
    assert soft_inf
    # a CRC that passes although the filler positions hold ones: they must take no part in it
    assert filler_ones == case.random_fillers
