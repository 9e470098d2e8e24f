"""Shared input generators for the LDPC parity tests (seeded, deterministic)."""
import collections
import functools

import numpy as np

import oracle


def noisy_codeblocks(bg, Z, n, length=None, snr_amp=10, noise=8.0, seed=0, crc_poly=None):
    """Encodes n random messages (optionally with a CRC appended to the message)
    and returns (messages [n, K] bits, llrs [n, length] int8)."""
    rng = np.random.default_rng(seed)
    K = oracle.BG_K[bg] * Z
    N = oracle.BG_N_SHORT[bg] * Z
    L = N if length is None else length
    msgs = np.zeros((n, K), np.uint8)
    llrs = np.zeros((n, L), np.int8)
    for i in range(n):
        m = rng.integers(0, 2, K).astype(np.uint8)
        if crc_poly is not None:
            L_crc = 24 if crc_poly in (0, 1, 2) else 16
            c = oracle.crc_bits(crc_poly, m[:K - L_crc])
            m[K - L_crc:] = [(c >> (L_crc - 1 - b)) & 1 for b in range(L_crc)]
        cw = oracle.ldpc_encode(m, bg, Z)[:L]
        x = (1 - 2 * cw.astype(np.float64)) * snr_amp + rng.normal(0, noise, L)
        llrs[i] = np.clip(np.round(x), -120, 120).astype(np.int8)
        msgs[i] = m
    return msgs, llrs


def crc_len(crc_poly):
    return 24 if crc_poly in (0, 1, 2) else 16


def _saturate(x, value):
    """x with every non-zero entry replaced by +-value, sign kept."""
    return (np.sign(x) * value).astype(np.int8)


def strong_codeblocks(bg, Z, n, seed, amp=40, noises=(20, 14, 24, 30, 34, 60), crc_poly=None, filler=0,
                      random_fillers=False):
    """Saturated inputs (HARQ-combined buffers, high-SNR demapper output): n full-length codeblocks whose LLRs take
    every valid reference value, [-120, 120] and +-127 (never 121..126 or -128).  Row i has noise noises[i mod len];
    a seeded 2 % of each row is pushed to +-127 with its sign kept.  The message's last ``filler`` bits are zero
    (+127 in the LLRs, as the rate dematcher writes them) and the CRC covers the K - filler - L_crc bits before them.
    random_fillers: the last ``filler`` bits are random message bits with ordinary LLRs instead, the input of a
    decoder that is told of filler bits the transmitter did not zero; the CRC still ends before them.
    Returns (messages [n, K] bits, llrs [n, N] int8)."""
    rng = np.random.default_rng(seed)
    K = oracle.BG_K[bg] * Z
    N = oracle.BG_N_SHORT[bg] * Z
    msgs = np.zeros((n, K), np.uint8)
    llrs = np.zeros((n, N), np.int8)
    for i in range(n):
        m = rng.integers(0, 2, K).astype(np.uint8)
        if not random_fillers:
            m[K - filler:] = 0
        if crc_poly is not None:
            L_crc = crc_len(crc_poly)
            c = oracle.crc_bits(crc_poly, m[:K - filler - L_crc])
            m[K - filler - L_crc:K - filler] = [(c >> (L_crc - 1 - b)) & 1 for b in range(L_crc)]
        cw = oracle.ldpc_encode(m, bg, Z)
        x = (1 - 2 * cw.astype(np.float64)) * amp + rng.normal(0, noises[i % len(noises)], N)
        x = np.clip(np.round(x), -120, 120).astype(np.int8)
        inf = rng.random(N) < 0.02
        x[inf] = _saturate(x[inf], 127)
        if filler and not random_fillers:
            x[K - 2 * Z - filler:K - 2 * Z] = 127  # LLR i is soft bit 2 Z + i
        llrs[i] = x
        msgs[i] = m
    return msgs, llrs


def force_tail_extremes(llrs, lens, Z):
    """In place: for every row whose length is not a multiple of Z, the first LLR of the partial tail node becomes
    +-127 and the last one +-120 (sign kept, zero counts as positive), so that every partial tail node holds a value
    that a clamp to +-64 would change.  A one-LLR tail gets +-127."""
    for i, L in enumerate(lens):
        if L % Z:
            first, last = (L // Z) * Z, L - 1
            llrs[i, last] = 120 if llrs[i, last] >= 0 else -120
            llrs[i, first] = 127 if llrs[i, first] >= 0 else -127
    return llrs


def ragged_lengths(bg, Z):
    """Six lengths from the shortest to the full codeblock: whole nodes, L mod Z in {1, 2, Z - 3, Z - 1, 7}."""
    lo = (24 if bg == 1 else 12) * Z
    N = oracle.BG_N_SHORT[bg] * Z
    return (N, lo + Z + 1, lo + 5 * Z - 1, N - 3, lo + 9 * Z + 2, N - Z + 7)


# One input set of the strong-input GPU tests (tests/test_ldpc_decoder_gpu.py); tests/test_ldpc_cases.py checks each
# against the oracle alone, so that no GPU test passes vacuously.  lens: per-row lengths; short: rows that keep only
# K - 1 leading LLRs (force_decoding rows, their length is a multiple of Z).
StrongCase = collections.namedtuple("StrongCase", "bg Z lens crc filler seed iters short noises random_fillers")


# Seeds chosen so that every case meets the conditions of tests/test_ldpc_cases.py (default: 1000 bg + Z).
SEEDS = {("par", 2, 7): 1, ("rag", 1, 36): 1, ("una", 1, 36, 0): 1, ("per", 1, 36): 2}
DEFAULT_NOISES = (20, 14, 24, 30, 34, 60)
# the shortest BG1 codeblocks (rate 22 / 24) decode at less noise only
HIGH_RATE_NOISES = (16, 14, 18, 15, 17, 60)


def _case(bg, Z, lens, crc, filler=0, seed=None, iters=8, short=(), noises=DEFAULT_NOISES, random_fillers=False):
    return StrongCase(bg, Z, tuple(lens), crc, filler, bg * 1000 + Z if seed is None else seed, iters, tuple(short),
                      tuple(noises), random_fillers)


def _uniform(bg, Z, L, crc, **kw):
    return _case(bg, Z, [L] * 6, crc, **kw)


def full_length(bg, Z):
    return oracle.BG_N_SHORT[bg] * Z


def min_length(bg, Z):
    return (24 if bg == 1 else 12) * Z


# (a) every kernel class: one row per lane (Z = 7, 26), packed with 1, 2, 3 waves, BG1 Z = 384 high-rate and full
PARITY_ZS = (7, 26, 36, 104, 144, 208, 352, 384)


def parity_cases():
    cases = []
    for bg in (1, 2):
        for Z in PARITY_ZS:
            crc = 1 if Z >= 26 else 3  # CRC24B, CRC16 for the smallest messages
            if (bg, Z) == (1, 384):
                cases.append(_uniform(bg, Z, min_length(bg, Z), crc, seed=SEEDS.get(("hr", bg, Z)),
                                      noises=HIGH_RATE_NOISES))
            cases.append(_uniform(bg, Z, full_length(bg, Z), crc, seed=SEEDS.get(("par", bg, Z))))
    return cases


# (b) ragged and unaligned rows
RAGGED_BZ = ((1, 36), (2, 36), (1, 208), (2, 208), (1, 352), (2, 352), (1, 384))


def unaligned_lengths(bg, Z):
    """Uniform lengths with L mod 4 = 1, 2, 3; the first has L mod Z = 1 and the last L mod Z = Z - 1."""
    lo = min_length(bg, Z)
    return (lo + 3 * Z + 1, lo + 12 * Z + 2, lo + 7 * Z - 1)


def ragged_case(bg, Z):
    return _case(bg, Z, ragged_lengths(bg, Z), 1, seed=SEEDS.get(("rag", bg, Z)))


def unaligned_cases(bg, Z):
    return [_uniform(bg, Z, L, 1, seed=SEEDS.get(("una", bg, Z, k))) for k, L in enumerate(unaligned_lengths(bg, Z))]


SOFT_OUT_CASES = ((1, 104, 66 * 104), (2, 104, 50 * 104), (1, 384, 24 * 384), (1, 384, 66 * 384))


def soft_out_case(bg, Z, L):
    return _uniform(bg, Z, L, 1, seed=SEEDS.get(("so", bg, Z, L)),
                    noises=HIGH_RATE_NOISES if L == min_length(bg, Z) else DEFAULT_NOISES)


# (c) CRC early stop with filler bits: (bg, Z, L, crc, F); K - F mod 4 = 3, 1, 1, 3, 1, 1, 1, 2, 2
FILLER_CASES = (
    (1, 104, 66 * 104, 1, 201),
    (2, 208, 50 * 208, 3, 7),
    (2, 384, 50 * 384, 1, 131),
    (1, 352, 66 * 352, 0, 1),
    (1, 384, 24 * 384, 1, 203),
    (1, 384, 66 * 384, 1, 203),
    (2, 64, 50 * 64, 3, 3),
    (1, 144, 66 * 144, 0, 6),
    (2, 36, 50 * 36, 3, 2),
)


def filler_case(bg, Z, L, crc, F, random_fillers=False):
    """random_fillers: message bits in the filler positions, so that the CRC passes only where the filler bits take
    no part in it (zero filler bits leave any CRC remainder as it is)."""
    return _uniform(bg, Z, L, crc, filler=F, seed=SEEDS.get(("fil", bg, Z, L)), random_fillers=random_fillers,
                    noises=HIGH_RATE_NOISES if L == min_length(bg, Z) else DEFAULT_NOISES)


# (d) persistent loop: 11 rows over 3 workgroups, long, short, long, short, so that every workgroup decodes a short
# row straight after a long one; row 4 keeps fewer than K LLRs (force_decoding: no decoding, no output)
PERSISTENT_BZ = ((2, 208), (2, 352), (1, 36), (2, 26))


def persistent_case(bg, Z):
    lo, N = min_length(bg, Z), full_length(bg, Z)
    lens = (N, N - 3, N - Z + 7,
            lo + Z + 1, lo + 2 * Z, lo + 5 * Z - 1,
            N - 1, N, N - 2 * Z + 2,
            lo + 2, lo + 3 * Z + Z // 2)
    # long rows that pass, fail late and fail; short rows that pass
    noises = (20, 30, 60, 14, 34, 16, 24, 14, 34, 15, 18)
    return _case(bg, Z, lens, 1 if Z >= 36 else 3, seed=SEEDS.get(("per", bg, Z)), short=(4,), noises=noises)


def all_cases():
    cases = parity_cases()
    for bg, Z in RAGGED_BZ:
        cases.append(ragged_case(bg, Z))
        cases += unaligned_cases(bg, Z)
    cases += [soft_out_case(*c) for c in SOFT_OUT_CASES]
    cases += [filler_case(*c, random_fillers=r) for c in FILLER_CASES for r in (False, True)]
    cases += [persistent_case(*c) for c in PERSISTENT_BZ]
    return list(dict.fromkeys(cases))


@functools.lru_cache(maxsize=None)
def _strong_inputs(case):
    n = len(case.lens)
    K = oracle.BG_K[case.bg] * case.Z
    msgs, llrs = strong_codeblocks(case.bg, case.Z, n, case.seed, noises=case.noises, crc_poly=case.crc,
                                   filler=case.filler, random_fillers=case.random_fillers)
    for i in case.short:
        assert case.lens[i] % case.Z == 0
        llrs[i, K - 1:] = 0
    force_tail_extremes(llrs, case.lens, case.Z)
    llrs.setflags(write=False)
    return msgs, llrs


def strong_inputs(case):
    """(messages [n, K], llrs [n, N] read-only) of a case: row i is valid up to case.lens[i], and the LLRs after it
    are those of the full codeblock, which a decoder must not read."""
    return _strong_inputs(case)
