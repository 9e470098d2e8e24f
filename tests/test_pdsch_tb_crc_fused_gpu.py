"""GPU parity: the TB CRC computed inside the PDSCH codeblock kernel (pdsch_encoder.hip).  Every non-last codeblock of
a segmented TB stores its contribution to the TB CRC, the TB's last codeblock (a second launch) XORs them with its own
and attaches the checksum.  Expected codewords come from oracle/sch.py (bit-exact with the reference's
pdsch_encoder_impl, tests/test_oracle_vs_ref.py) and, for the headline plan, from the compiled reference itself.
Bar: bit-exact, no tolerance."""
import numpy as np
import pytest

import oracle.sch as osch
from tests.sch_cases import tb_bytes

pytestmark = pytest.mark.gpu

# (tbs, base graph, Qm, layers, channel symbols): the smallest plans at which the in-kernel TB CRC can go wrong
CASES = [
    (8 * 1056, 1, 6, 1, 2000),    # C = 2, cb_info_bits 4236 (mod 8 = 4): one partial plus last, unaligned segment
    (8 * 1055, 1, 4, 1, 3000),    # C = 2, cb_info_bits 4232: byte-aligned segments
    (8 * 2113, 1, 4, 1, 6000),    # C = 3, cb_info_bits 5643 (mod 8 = 3), zero pad 1 after the TB CRC
    (8 * 3001, 2, 6, 2, 12000),   # BG2 C = 7, cb_info_bits 3434 (mod 8 = 2), zero pad 6, six partials
    (8 * 12000, 1, 2, 2, 96000),  # C = 12, cb_info_bits 8002, Z = 384
    (8 * 479, 2, 4, 1, 1400),     # C = 2, cb_info_bits 1928: the first TBS past the CRC16 boundary (3824 bits)
    (8 * 481, 2, 4, 1, 1400),     # C = 2, cb_info_bits 1936
    (8 * 500, 1, 4, 1, 1800),     # C = 1, CRC24A
    (8 * 478, 2, 4, 1, 1400),     # C = 1, CRC16 at its largest TBS: the TB CRC computed in the codeblock itself
]
# (C, cb_info_bits, zero_pad) of each case; cb_info_bits / zero_pad of a single segment are not pinned
GEOMETRY = [(2, 4236, 0), (2, 4232, 0), (3, 5643, 1), (7, 3434, 6), (12, 8002, 0), (2, 1928, 0), (2, 1936, 0),
            (1, None, None), (1, None, None)]
C12, C2, C7 = 4, 0, 3


@pytest.fixture(scope="module")
def enc():
    import srsran_project_amd as amd

    return amd.PdschEncoder()


def _plan(case):
    import srsran_project_amd as amd

    tbs, bg, qm, lay, nre = case
    p, op = amd.sch_plan(tbs, bg, 0, qm, 0, lay, nre), osch.plan(tbs, bg, 0, qm, 0, lay, nre)
    assert p.as_dict() == op
    return p, op


def _check_batch(enc, p, op, rows, what=""):
    """rows [n][tbs / 8] through encode_batch in padded rows, each against the oracle."""
    import torch

    n, nb = rows.shape
    padded = np.zeros((n, nb + 13), np.uint8)
    padded[:, :nb] = rows
    out = enc.encode_batch(torch.from_numpy(padded).cuda(), p)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k in range(n):
        np.testing.assert_array_equal(np.unpackbits(got[k])[:p.cw_length], osch.pdsch_encode(rows[k], op),
                                      err_msg="%sTB %d" % (what, k))


def _rows(tbs, seed, n=5):
    return np.stack([tb_bytes(tbs, seed + k) for k in range(n)])


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_plan_geometry(ci):
    """The cases exercise what they are listed for."""
    op = osch.plan(CASES[ci][0], CASES[ci][1], 0, CASES[ci][2], 0, CASES[ci][3], CASES[ci][4])
    C, cbi, zp = GEOMETRY[ci]
    assert op["nof_segments"] == C
    if C > 1:
        assert (op["cb_info_bits"], op["zero_pad"]) == (cbi, zp)
    assert op["nof_tb_crc_bits"] == (16 if CASES[ci][0] <= 3824 else 24)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_batch(enc, ci):
    """5 TBs in padded rows through encode_batch."""
    p, op = _plan(CASES[ci])
    _check_batch(enc, p, op, _rows(p.tbs, 1000 * ci + 17))


def _check_slot(enc, order, seed):
    import torch

    ues, tpos, cpos = [], 0, 0
    for u, ci in enumerate(order):
        p, op = _plan(CASES[ci])
        ues.append((p, tpos, cpos, op, tb_bytes(p.tbs, seed + u)))
        tpos += p.tbs // 8
        cpos += (p.cw_length + 7) // 8
    flat = np.concatenate([u[4] for u in ues] + [np.zeros(16, np.uint8)])
    out = torch.full((cpos + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    enc.encode_slot(torch.from_numpy(flat).cuda(), [(u[0], u[1], u[2]) for u in ues], out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for u, (p, _, co, op, tb) in enumerate(ues):
        bits = np.unpackbits(got[co:co + (p.cw_length + 7) // 8])
        np.testing.assert_array_equal(bits[:p.cw_length], osch.pdsch_encode(tb, op),
                                      err_msg="UE %d (case %d)" % (u, order[u]))
        assert not bits[p.cw_length:].any(), "UE %d: padding bits" % u
    assert (got[cpos:] == 0xA5).all(), "bytes after the codewords written"


def test_slot_mixed_then_single_codeblock_only(enc):
    """One encode_slot call mixes all the plans, single-codeblock TBs between segmented ones; a second call holds
    only single-codeblock TBs (no launch of non-last codeblocks)."""
    _check_slot(enc, [4, 8, 0, 2, 7, 3, 1, 8, 6, 5], 300)
    _check_slot(enc, [8, 7, 7, 8], 400)


def test_stale_partials():
    """C = 12, then C = 2, then C = 12 with other TB bytes on one encoder: the partials buffer is reused and nothing
    may depend on what an earlier call left there."""
    import srsran_project_amd as amd

    e = amd.PdschEncoder()
    p12, op12 = _plan(CASES[C12])
    p2, op2 = _plan(CASES[C2])
    _check_batch(e, p12, op12, _rows(p12.tbs, 5000), "first C = 12: ")
    _check_batch(e, p2, op2, _rows(p2.tbs, 5100), "C = 2: ")
    _check_batch(e, p12, op12, _rows(p12.tbs, 5200), "second C = 12: ")


@pytest.mark.parametrize("wg", ["64", "256"])
def test_tail_forms(enc, wg, monkeypatch):
    """The TBs' last codeblocks by one wave and by four waves (the default) per codeblock (SRSRAN_AMD_PDSCH_TAIL_WG),
    C = 7."""
    monkeypatch.setenv("SRSRAN_AMD_PDSCH_TAIL_WG", wg)
    p, op = _plan(CASES[C7])
    _check_batch(enc, p, op, _rows(p.tbs, 6000 + int(wg)))


def test_headline_plan_against_reference(enc):
    """The 4-layer PDSCH plan of the headline pipeline (256QAM, R = 948/1024, 273 PRB, 11 data symbols), one TB,
    against the compiled reference encoder."""
    import torch

    import oracle
    import srsran_project_amd as amd
    from bench_pipeline import DL_LAYERS, DL_NSYM, NPRB, QM, RATE, base_graph

    if oracle.REF is None:
        pytest.skip("reference library not built (oracle/_ref/libsrsran_ref.so)")
    tbs = amd.tbs_calculator_calculate(DL_NSYM, 24, 0, QM, RATE, DL_LAYERS, 0, NPRB)
    bg = base_graph(tbs, RATE / 1024)
    nre = NPRB * 12 * (DL_NSYM - 2) * DL_LAYERS
    p, op = amd.sch_plan(tbs, bg, 0, QM, 0, DL_LAYERS, nre), osch.plan(tbs, bg, 0, QM, 0, DL_LAYERS, nre)
    assert p.as_dict() == op
    assert p.nof_segments - 1 > 64  # more partials than one wave reads in a pass
    tb = tb_bytes(tbs, 4242)
    out = enc.encode_batch(torch.from_numpy(tb[None]).cuda(), p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np.unpackbits(out[0].cpu().numpy())[:p.cw_length], oracle.ref_pdsch_encode(tb, op))


def test_more_codeblocks_than_workgroups(enc):
    """A uniform batch of the C = 12 plan whose 4807 codeblocks but the TBs' last ones exceed the workgroups resident
    on the device (4096 on the MI355X: 16 per CU by the kernel's LDS) and are no multiple of them, so workgroups loop
    over several codeblocks; the TB bytes cycle over 3 TBs, every row against the oracle's codeword of its TB."""
    import torch

    p, op = _plan(CASES[C12])
    n = 437
    three = _rows(p.tbs, 7000, 3)
    want = [np.packbits(osch.pdsch_encode(three[k], op)) for k in range(3)]
    rows = torch.from_numpy(three).cuda()[torch.arange(n, device="cuda") % 3]
    out = enc.encode_batch(rows, p)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    nb = (p.cw_length + 7) // 8
    for k in range(n):
        assert np.array_equal(got[k, :nb], want[k % 3]), "TB %d" % k
