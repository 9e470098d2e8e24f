"""GPU parity of the estimator-fused PUSCH equalizer (pusch_equalize_fused_kernel<P, L, MMSE, MULTI>, the bench
path) at every instantiation and modulation, at LLR level.

Batch form (MULTI = false): the run without a caller estimate buffer (fused) against the run that writes and
re-reads the expanded estimates -- LLRs, transport blocks and result records bit-identical -- and both against
the reference demodulator (pusch_demodulator_impl for the topologies its equalizer implements, the fp64
restatement for the rest) fed the GPU's own estimates and port noise variances, so the pair is anchored outside
the code under test.  The allocation starts at CRB 5 of a 52-PRB grid (the estimator index kk differs from the
grid subcarrier), spans 276 subcarriers (two tiles, the second with 20 subcarriers of work), 12 of the 14 OFDM
symbols, and runs as 5 grids: 10 tiles in 16 tile slots, so the tile >= nof_tiles exit and the second round of
the XCD order both run.

Slot form (MULTI = true): PDUs of every ZF topology (then every MMSE topology) in one slot call with different
symbol counts and spans -- two groups hold PDUs whose own block count is below the launch's max_blocks --
against process_batch on the same grid and, for the topologies the compiled pusch_processor_impl runs, against
it.  The slot form has no LLR output in the C-ABI, so its LLRs stay unpinned: transport blocks, CRC flags and
LDPC iteration statistics are what is compared.
"""
import numpy as np
import pytest

import oracle
import srsran_project_amd as amd
from oracle import pusch_demod as od
from oracle import pusch_proc as pp
from tests.pusch_demod_cases import assert_llrs_close

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(oracle.REF is None, reason="oracle/_ref not built")]

# the kernel's instantiations (launch_pusch_equalize_fused): (ports, layers, MMSE)
ZF_TOPOLOGIES = [(1, 1, 0), (2, 1, 0), (4, 1, 0), (2, 2, 0), (4, 2, 0), (4, 3, 0), (4, 4, 0)]
MMSE_TOPOLOGIES = [(2, 2, 1), (4, 2, 1), (4, 3, 1), (4, 4, 1)]
PARAMS = [(P, L, eq, qm) for (P, L, eq) in ZF_TOPOLOGIES + MMSE_TOPOLOGIES for qm in (2, 4, 6, 8)] + [(2, 1, 0, 1)]

NPRB = 52
NSUBC = 12 * NPRB
SENTINEL = -77
# inside the allocation (CRBs 5 to 27), in the second tile, an odd subcarrier of its PRB: a data RE on every symbol
DC = 60 + 256 + 5
RATE = 120.0  # target code rate x 1024 (MCS table 1 index 1), low enough that every transport block decodes
# SNR per layer after combining; each sits several dB above the decoding threshold of its modulation at this rate and
# well below the SNR at which the LLRs saturate, so that the compared LLRs carry information
SNR_DB = {1: 2.0, 2: 2.0, 4: 5.0, 6: 8.0, 8: 10.0}

BASE = dict(numerology=1, slot_index=3, rv=0, new_data=1, dmrs_type=1, n_scid=0, tbs_lbrm_bytes=0)


def _chan(L, P, seed):
    rng = np.random.default_rng(seed)
    h = np.eye(L, P) + 0.25 * (rng.normal(size=(L, P)) + 1j * rng.normal(size=(L, P)))
    return (0.8 * h).astype(np.complex64)


def _finish(pdu):
    """Transport block size and base graph of a PDU dict."""
    ndmrs = 6 * bin(pdu["dmrs_symbol_mask"]).count("1") * pdu["nof_cdm_groups_without_data"]
    qm, rate = pdu["modulation"], pdu["target_code_rate"]
    if qm == 1:  # the calculator takes Qm >= 2: the same N_info = N_RE R Qm v from QPSK at half the rate
        qm, rate = 2, rate / 2
    tbs = amd.tbs_calculator_calculate(pdu["nof_symbols"], ndmrs, 0, qm, rate, pdu["nof_tx_layers"], 0,
                                       pdu["rb_count"])
    r = pdu["target_code_rate"] / 1024
    pdu["base_graph"] = 2 if (tbs <= 292 or (tbs <= 3824 and r <= 0.67) or r <= 0.25) else 1
    pdu["tbs"] = tbs
    return pdu


def _snr(qm, P, L):
    """SNR of the received grid (all layers' power over the noise of one port) that gives each layer about
    SNR_DB[qm] after a linear equalizer of diversity order P - L + 1."""
    return SNR_DB[qm] + 10 * np.log10(L / (P - L + 1))


def _batch_case(idx):
    """PDU, DC position and time-domain strategy of parametrisation idx."""
    P, L, eq, qm = PARAMS[idx]
    dc = DC if idx % 2 else None
    td = (idx // 2) % 2  # interpolate, interpolate, average, average, ...: each topology has both, with and without DC
    pdu = _finish(dict(BASE, rnti=0x4601 + idx, n_id=100 + idx, scrambling_id=7 + idx, bwp_start_rb=2, bwp_size_rb=50,
                       rb_start=3, rb_count=23, start_symbol_index=1, nof_symbols=12,
                       dmrs_symbol_mask=(1 << 2) | (1 << 7), nof_cdm_groups_without_data=1 if L <= 2 else 2,
                       modulation=qm, target_code_rate=RATE, nof_tx_layers=L, nof_rx_ports=P))
    return pdu, dc, td


def _batch_grid(idx, pdu, i):
    """Transport block and received grid i of parametrisation idx."""
    P, L, eq, qm = PARAMS[idx]
    tb = np.random.default_rng(1000 * idx + i).integers(0, 256, pdu["tbs"] // 8, dtype=np.uint8)
    return tb, pp.ue_transmit(tb, pdu, NSUBC, channel=_chan(L, P, 50 + idx), snr_db=_snr(qm, P, L), seed=i)[0]


@pytest.mark.parametrize("idx", range(len(PARAMS)), ids=["%dx%d_%s_qm%d" % (p[0], p[1], ("zf", "mmse")[p[2]], p[3])
                                                          for p in PARAMS])
def test_fused_equalizer_llrs_every_topology(idx):
    """LLRs, transport blocks, results and port measurements of 5 grids bit-identical with and without a caller
    estimate buffer, nothing written beyond the codeword, every transport block the transmitted one, and the LLRs
    within assert_llrs_close of the reference demodulator on the returned estimates and noise variances."""
    import torch

    P, L, eq, qm = PARAMS[idx]
    pdu, dc, td = _batch_case(idx)
    n = 5
    sent, grids = zip(*[_batch_grid(idx, pdu, i) for i in range(n)])
    grids = np.stack(grids)
    proc = amd.PuschProcessor(amd.PuschProcessorConfig(dec_nof_iterations=6, td_interpolation=td, equalizer=eq),
                              device=0)
    plan = proc.plan(amd.make_pdu(**dict(pdu, dc_position=dc)), NSUBC)
    crbs = list(range(5, 28))
    mask = od.data_re_mask(NSUBC, crbs, 1, 12, pdu["dmrs_symbol_mask"], False, pdu["nof_cdm_groups_without_data"])
    G = plan.sch.cw_length
    assert G == int(mask.sum()) * L * qm
    g = torch.from_numpy(grids.view(np.int32)).to("cuda:0")
    got = []
    for keep in (True, False):
        est = torch.zeros((n, P, L, 14, NSUBC), dtype=torch.int32, device="cuda:0") if keep else None
        st = torch.zeros((n, P, 6), dtype=torch.float32, device="cuda:0")
        llrs = torch.full((n, (G + 63) // 64 * 64 + 64), SENTINEL, dtype=torch.int8, device="cuda:0")
        out, res = proc.process_batch(g, plan, estimates=est, llrs=llrs, port_stats=st)
        torch.cuda.synchronize()
        got.append((llrs.cpu().numpy(), out.cpu().numpy(), res.cpu().numpy(), st.cpu().numpy(),
                    None if est is None else est.cpu().numpy().view(np.uint32)))
    # fused == expanded, bit for bit; nothing written past the codeword
    for a, b, what in zip(got[0][:4], got[1][:4], ("LLRs", "transport blocks", "results", "port measurements")):
        assert np.array_equal(a, b), what
    for run in got:
        assert (run[0][:, G:] == SENTINEL).all(), "LLR row written beyond the codeword"
    res = amd.pusch_processor.parse_results(got[1][2])
    for i in range(n):
        assert res[i].data.tb_crc_ok and np.array_equal(got[1][1][i], sent[i]), "grid %d" % i
    # ... and both equal the reference demodulator on the GPU's own estimates and noise variances
    est, st = got[0][4], got[0][3]
    if dc is not None:
        assert (est[:, :, :, 1:13, DC] == 0).all() and (est[:, :, :, 1:13, DC + 1] != 0).all()
    a = dict(qm=qm, crbs=crbs, start_symbol=1, nof_symbols=12, dmrs_symb_mask=pdu["dmrs_symbol_mask"],
             dmrs_type2=False, nof_cdm_groups_without_data=pdu["nof_cdm_groups_without_data"], nof_layers=L)
    for i in range(n):
        if eq == 0 and L <= 2:
            want = od.ref_pusch_demodulate(grids[i], est[i], st[i, :, 0], pdu["rnti"], pdu["n_id"], **a)
        else:
            want = od.pusch_demodulate(grids[i], est[i], st[i, :, 0], pdu["rnti"], pdu["n_id"], mmse=bool(eq), **a)
        assert_llrs_close(got[1][0][i, :G], want, "grid %d LLRs" % i)


# One slot on a four-port 106-PRB grid: a PDU of every topology on disjoint PRBs (receive ports 0 .. P - 1), with
# 14, 12 and 9 OFDM symbols and spans of one and three tiles.  The (2, 1) and (4, 2) groups hold two PDUs each, whose
# block counts differ (8 x 12 and 8 x 9 symbols), so blocks beyond a PDU's own count run.
# (ports, layers, rb_start, rb_count, start symbol, nof symbols, DM-RS symbols, modulation)
SLOT_PDUS = [
    (1, 1, 0, 6, 0, 14, (1 << 2) | (1 << 11), 2),
    (2, 1, 6, 8, 1, 12, (1 << 2) | (1 << 11), 4),
    (4, 1, 14, 5, 2, 9, (1 << 3) | (1 << 8), 6),
    (2, 2, 19, 6, 0, 14, (1 << 2) | (1 << 11), 4),
    (4, 2, 25, 43, 1, 12, (1 << 2) | (1 << 11), 6),
    (4, 3, 68, 8, 2, 9, (1 << 3) | (1 << 8), 2),
    (4, 4, 76, 10, 0, 14, (1 << 2) | (1 << 11), 4),
    (2, 1, 86, 4, 2, 9, (1 << 3), 2),
    (4, 2, 90, 5, 2, 9, (1 << 3) | (1 << 8), 4),
]
SLOT_NPRB = 106
SLOT_RATE = {2: 308.0, 4: 340.0, 6: 378.0}  # x 1024; the slot is received at 30 dB


def _to_complex(g):
    f = np.stack([((g & 0xFFFF) << 16).view(np.float32), ((g >> 16) << 16).view(np.float32)], -1)
    return f[..., 0] + 1j * f[..., 1]


def _from_complex(z):
    from oracle.pdsch_mod import to_bf16
    return np.ascontiguousarray(to_bf16(z.real.astype(np.float32)).astype(np.uint32)
                                | (to_bf16(z.imag.astype(np.float32)).astype(np.uint32) << 16))


def _slot_case():
    """The received four-port grid of the slot, its PDUs and their transport blocks."""
    pdus, sent = [], []
    z = 0
    for u, (P, L, rb0, nrb, s0, ns, dmrs, qm) in enumerate(SLOT_PDUS):
        pdu = _finish(dict(BASE, rnti=0x5001 + u, n_id=10 + u, scrambling_id=20 + u, n_scid=u % 2, bwp_start_rb=0,
                           bwp_size_rb=SLOT_NPRB, rb_start=rb0, rb_count=nrb, start_symbol_index=s0, nof_symbols=ns,
                           dmrs_symbol_mask=dmrs, nof_cdm_groups_without_data=1 if L <= 2 else 2, modulation=qm,
                           target_code_rate=SLOT_RATE[qm], nof_tx_layers=L, nof_rx_ports=P))
        tb = np.random.default_rng(70 + u).integers(0, 256, pdu["tbs"] // 8, dtype=np.uint8)
        g, _ = pp.ue_transmit(tb, pdu, 12 * SLOT_NPRB, channel=_chan(L, 4, 30 + u), nof_rx_ports=4)
        z = z + _to_complex(g)
        pdus.append(pdu)
        sent.append(tb)
    occ = np.abs(z) > 0
    sigma = np.sqrt(float(np.mean(np.abs(z[occ]) ** 2)) / 10 ** (30.0 / 10) / 2)
    rng = np.random.default_rng(9)
    grid = _from_complex(z + sigma * (rng.normal(size=z.shape) + 1j * rng.normal(size=z.shape)))
    return grid, pdus, sent


@pytest.fixture(scope="module")
def slot_case():
    return _slot_case()


@pytest.mark.parametrize("eq", [0, 1], ids=["zf", "mmse"])
def test_fused_slot_form_every_topology(slot_case, eq):
    import torch

    grid, pdus, sent = slot_case
    iters = 6
    # MMSE: the PDUs of the four MMSE instantiations (one layer is the ZF kernel whatever the algorithm)
    pick = [u for u, p in enumerate(pdus) if eq == 0 or p["nof_tx_layers"] >= 2]
    assert sorted({(pdus[u]["nof_rx_ports"], pdus[u]["nof_tx_layers"], eq) for u in pick}) == \
        sorted(ZF_TOPOLOGIES if eq == 0 else MMSE_TOPOLOGIES)
    proc = amd.PuschProcessor(amd.PuschProcessorConfig(dec_nof_iterations=iters, equalizer=eq), device=0)
    plans = [proc.plan(amd.make_pdu(**pdus[u]), 12 * SLOT_NPRB) for u in pick]
    g = torch.from_numpy(grid.view(np.int32)[None]).to("cuda:0")
    out, offs, res = proc.process_slot(g, [(pl, 0) for pl in plans])
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    res = amd.pusch_processor.parse_results(res.cpu().numpy())
    for k, (u, pl) in enumerate(zip(pick, plans)):
        pdu = pdus[u]
        tag = "pdu %d (%d x %d)" % (u, pdu["nof_rx_ports"], pdu["nof_tx_layers"])
        got_tb = out[offs[k]:offs[k] + pl.tb_bytes]
        assert res[k].data.tb_crc_ok and np.array_equal(got_tb, sent[u]), tag
        b_tb, b_res = proc.process_batch(g, pl)
        torch.cuda.synchronize()
        b = amd.pusch_processor.parse_results(b_res.cpu().numpy())[0]
        assert np.array_equal(b_tb[0].cpu().numpy(), got_tb), tag
        assert b.data.tb_crc_ok == res[k].data.tb_crc_ok, tag
        assert b.data.ldpc_iterations_sum == res[k].data.ldpc_iterations_sum, tag
        assert b.data.ldpc_iterations_max == res[k].data.ldpc_iterations_max, tag
        for f in ("sinr_db", "epre_db", "rsrp_db", "time_alignment_s", "cfo_hz"):
            x, y = getattr(b, f), getattr(res[k], f)
            assert x == y or (np.isnan(x) and np.isnan(y)), (tag, f, x, y)
        if eq == 0 and pdu["nof_tx_layers"] <= 2:
            want_tb, want = pp.ref_pusch_process(grid[:pdu["nof_rx_ports"]], pdu, pl.tb_bytes, iterations=iters)
            assert bool(res[k].data.tb_crc_ok) == want["tb_crc_ok"], tag
            assert np.array_equal(got_tb, want_tb), tag
            assert res[k].data.nof_codeblocks_total == want["nof_codeblocks_total"], tag
            assert res[k].data.ldpc_iterations_sum == want["iterations_sum"], (tag, res[k].data.ldpc_iterations_sum,
                                                                              want)
            assert res[k].data.ldpc_iterations_max == want["iterations_max"], tag
            for f in ("sinr_db", "epre_db", "rsrp_db"):
                assert abs(getattr(res[k], f) - want[f]) <= 0.05, (tag, f, getattr(res[k], f), want[f])
            assert abs(res[k].time_alignment_s - want["time_alignment_s"]) <= 2e-9, tag
