"""NZP-CSI-RS generator on the MI355X (srs_amd_csi_rs_map / srs_amd_csi_rs_map_slot through the Python layer).

References: the grids recorded from the reference's own generator (tests/golden/csi_rs_golden.npz, written by
tools/csi_rs_golden_gen.cpp; the "auto" precoder of the recording machine, and the REs where the "generic" precoder
wrote other bits -- both are the reference) and the numpy model written from TS 38.211 (tests/csi_rs_model.py).  The
GPU is never compared with itself for accuracy; the batch / stream tests compare raw grids of the same deterministic
kernel for identity.

Every grid the GPU sees starts as seeded non-zero garbage in every RE, the ports a resource does not have and grid
ports beyond the row's included: at the REs of the pattern the bits must be the reference's, every other RE must still
hold the garbage.  Everything here is bit-exact; there is no tolerance.
"""
import numpy as np
import pytest

from tests import csi_rs_model as cm

pytestmark = pytest.mark.gpu

FIXTURES = cm.fixtures()
IDS = [fx.name for fx in FIXTURES]


@pytest.fixture(scope="module")
def gen(device):
    import srsran_project_amd as amd

    g = amd.CsiRsGenerator(device.index or 0)
    yield g
    g.close()


def _to_device(grids, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(grids).view(np.int16)).to(device)


def _to_host(t):
    return t.cpu().numpy().view(np.uint16)


def _pad_ports(a, nof_ports):
    out = np.zeros((nof_ports,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def _check_fixture(got, garbage, fx, label):
    """got, garbage: [ports, 14, nof_subc, 2] with at least the fixture's ports."""
    ports = got.shape[0]
    _, mask = fx.model()
    mask = _pad_ports(mask, ports)
    auto, generic = _pad_ports(fx.reference(), ports), _pad_ports(fx.reference(generic=True), ports)
    assert mask.any()
    ok = (got[mask] == auto[mask]).all(axis=-1) | (got[mask] == generic[mask]).all(axis=-1)
    assert ok.all(), "%s: %d of %d pattern REs differ from the reference" % (label, int((~ok).sum()), ok.size)
    assert np.array_equal(got[~mask], garbage[~mask]), "%s: an RE outside the pattern was written" % label


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_host_form(gen, fx):
    # one grid port more than the row needs
    garbage = cm.garbage_grid(1, fx.nof_grid_ports + 1, fx.nof_subc, 100 + len(fx.name))[0]
    got = garbage
    for c in fx.cfgs:
        got = gen.map(got, c.library())
    _check_fixture(got, garbage, fx, fx.name)


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_slot_form(gen, device, fx):
    """All resources of the fixture in ONE map_slot call (the multi case: a TRS slot plus a row-4 resource), on the
    second of three grids; the other grids stay garbage."""
    import torch

    garbage = cm.garbage_grid(3, fx.nof_grid_ports, fx.nof_subc, 200 + len(fx.name))
    g = _to_device(garbage, device)
    gen.map_slot(g, [c.library(grid=1) for c in fx.cfgs])
    torch.cuda.synchronize()
    got = _to_host(g)
    _check_fixture(got[1], garbage[1], fx, fx.name)
    assert np.array_equal(got[0], garbage[0]) and np.array_equal(got[2], garbage[2])


def _perm(n, shift=1):
    w = np.zeros((n, n), np.complex64)
    for i in range(n):
        w[i, (i + shift) % n] = 1.0
    return w


FRESH = [
    cm.Config(row=1, k_ref=[2], symbol_l0=9, start_rb=17, nof_rb=33, cdm=cm.CDM_NONE, freq_density=cm.D_THREE,
              scrambling_id=77, amplitude=0.7, numerology=1, slot_index=5),
    cm.Config(row=2, k_ref=[7], symbol_l0=1, start_rb=21, nof_rb=30, cdm=cm.CDM_NONE, freq_density=cm.D_ODD,
              scrambling_id=901, amplitude=1.0, numerology=2, slot_index=39),
    cm.Config(row=3, k_ref=[6], symbol_l0=11, start_rb=5, nof_rb=61, cdm=cm.CDM_FD2, freq_density=cm.D_ONE,
              scrambling_id=3, amplitude=1.9, numerology=1, slot_index=12, weights=_perm(2)),
    cm.Config(row=4, k_ref=[4], symbol_l0=13, start_rb=33, nof_rb=41, cdm=cm.CDM_FD2, freq_density=cm.D_ONE,
              scrambling_id=555, amplitude=1.0, numerology=0, slot_index=9),
    cm.Config(row=5, k_ref=[9], symbol_l0=3, start_rb=1, nof_rb=99, cdm=cm.CDM_FD2, freq_density=cm.D_ONE,
              scrambling_id=1000, amplitude=0.31, numerology=3, slot_index=64, weights=_perm(4, 3)),
]


def test_fresh_configurations_against_the_model(gen, device):
    import torch

    ports, subc = 4, 106 * 12
    garbage = cm.garbage_grid(len(FRESH), ports, subc, 31)
    g = _to_device(garbage, device)
    gen.map_slot(g, [c.library(grid=i) for i, c in enumerate(FRESH)])
    torch.cuda.synchronize()
    got = _to_host(g)
    for i, c in enumerate(FRESH):
        assert cm.one_nonzero_weight_per_port(c)
        bits, mask = cm.model_grid([c], ports, subc, base=garbage[i])
        assert mask[:c.nof_ports].any() and not mask[c.nof_ports:].any()
        assert np.array_equal(got[i], bits), "fresh configuration %d (row %d)" % (i, c.row)
        assert np.array_equal(got[i][~mask], garbage[i][~mask])


def _mixed_resources(nof_grids):
    """(grid, Config) of a slot: four kinds of cells, all on 52 PRB x 4 ports."""
    kinds = [
        [cm.Config(row=1, k_ref=[1], symbol_l0=4, start_rb=0, nof_rb=52, freq_density=cm.D_THREE, scrambling_id=33),
         cm.Config(row=1, k_ref=[1], symbol_l0=8, start_rb=0, nof_rb=52, freq_density=cm.D_THREE, scrambling_id=33),
         cm.Config(row=4, k_ref=[4], symbol_l0=13, start_rb=0, nof_rb=52, cdm=cm.CDM_FD2, scrambling_id=34)],
        [cm.Config(row=5, k_ref=[2], symbol_l0=5, start_rb=3, nof_rb=47, cdm=cm.CDM_FD2, scrambling_id=35,
                   weights=_perm(4, 2))],
        [cm.Config(row=3, k_ref=[8], symbol_l0=0, start_rb=1, nof_rb=51, cdm=cm.CDM_FD2, freq_density=cm.D_EVEN,
                   scrambling_id=36, amplitude=2.0),
         cm.Config(row=2, k_ref=[11], symbol_l0=13, start_rb=0, nof_rb=51, freq_density=cm.D_ODD, scrambling_id=37)],
        [cm.Config(row=1, k_ref=[3], symbol_l0=12, start_rb=50, nof_rb=2, freq_density=cm.D_THREE, scrambling_id=38,
                   weights=np.array([[0.5 - 0.5j]])),
         cm.Config(row=3, k_ref=[0], symbol_l0=2, start_rb=10, nof_rb=9, cdm=cm.CDM_FD2, scrambling_id=39,
                   weights=np.array([[0.3 + 0.1j, -0.7j], [0.25, 1.0 - 0.5j]]))],
    ]
    out = []
    for g in range(nof_grids):
        for c in kinds[g % len(kinds)]:
            out.append((g, cm.Config(**{**c.__dict__, "slot_index": (c.slot_index + g) % 20})))
    return out


def test_64_grids_equal_one_at_a_time_and_do_not_synchronise(gen, device):
    """One map_slot call over 64 grids of mixed rows against the same resources mapped one at a time, in reversed
    order, through d_grid, on a second stream: raw identity.  The 64-grid call is issued into a stream that a long
    kernel occupies: it returns while that kernel still runs (no host synchronisation) and completes after it."""
    import torch

    nof_grids, ports, subc = 64, 4, 624
    garbage = cm.garbage_grid(nof_grids, ports, subc, 77)
    resources = _mixed_resources(nof_grids)
    cfgs = [c.library(grid=g) for g, c in resources]

    # The descriptor scratch grows to a call's size the first time it is met: the device buffer on the first call, each
    # of the three pinned staging buffers of the ring on its own first use (growing one frees the smaller buffer, which
    # waits for the device).  A cell's resources are static, so the steady state is what the claim is about.
    warm = _to_device(garbage, device)
    for _ in range(3):
        gen.map_slot(warm, cfgs)
    torch.cuda.synchronize()

    batch = _to_device(garbage, device)
    a = torch.randn((8192, 8192), device=device)
    _ = a @ a  # the BLAS library's own start-up happens here, not inside the timed stream
    s1 = torch.cuda.Stream(device)
    long_done = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        b = a
        for _ in range(16):
            b = (b @ a) * 1e-2
        long_done.record(s1)
        gen.map_slot(batch, cfgs, stream=s1)
        returned_while_busy = not long_done.query()
    assert returned_while_busy, "map_slot returned only after the work queued in front of it"
    s1.synchronize()
    assert long_done.query()
    assert torch.equal(batch, warm)

    single = _to_device(garbage, device)
    s2 = torch.cuda.Stream(device)
    grid_bytes = ports * 14 * subc * 4
    with torch.cuda.stream(s2):
        for g, c in reversed(resources):
            gen.map_slot(single, [c.library(grid=0, d_grid=single.data_ptr() + g * grid_bytes)], stream=s2)
    s2.synchronize()
    assert torch.equal(batch, single)
    # and the grids are the model's (identity / permutation resources) with the garbage kept elsewhere
    got = _to_host(batch)
    for g in (0, 1, 2, 63):
        mine = [c for gg, c in resources if gg == g]
        bits, mask = cm.model_grid(mine, ports, subc, base=garbage[g])
        assert np.array_equal(got[g][~mask], garbage[g][~mask])
        if all(cm.one_nonzero_weight_per_port(c) for c in mine):
            assert np.array_equal(got[g], bits)
        else:
            assert cm.bf16_ulp_distance(got[g][mask], bits[mask]).max() <= 1


def test_pdsch_reserves_the_csi_rs_res(gen, device):
    """One grid, one PDSCH PDU through modulate_slot whose reserved REs are csi_rs_reserved(cfg), then map_slot of
    cfg: the CSI-RS REs are the model's, every other RE is the PDSCH-only grid, and the reservation changed what the
    PDSCH wrote."""
    import torch

    import srsran_project_amd as amd

    ports, nprb = 2, 52
    subc = 12 * nprb
    cfg = cm.Config(row=3, k_ref=[5], symbol_l0=6, start_rb=7, nof_rb=38, cdm=cm.CDM_FD2, freq_density=cm.D_ONE,
                    scrambling_id=321, amplitude=1.0, numerology=1, slot_index=11)
    reserved = amd.csi_rs_reserved(cfg.library())
    assert len(reserved) == 1
    garbage = cm.garbage_grid(1, ports, subc, 5)
    mod = amd.PdschModulator(device=device.index or 0)
    W = (np.array([[0.6 + 0.2j, -0.3 + 0.5j]]) / np.sqrt(2)).astype(np.complex64)

    def pdsch(res):
        return amd.PdschModulatorConfig(rnti=4601, bwp_start=0, bwp_size=nprb, modulation=4, crbs=list(range(nprb)),
                                        start_symbol=1, nof_symbols=13, dmrs_symb_pos=1 << 2, n_id=17, reserved=res,
                                        precoding=W)

    plan_res, plan_all = mod.plan(pdsch(reserved), subc), mod.plan(pdsch([]), subc)
    nof_csi_res = len(cm.pattern_res(cfg))
    assert plan_all.nof_re - plan_res.nof_re == nof_csi_res == 2 * 38
    cw = np.packbits(np.random.default_rng(8).integers(0, 2, plan_all.nof_bits).astype(np.uint8))

    def run(plan, with_csi_rs):
        g = torch.from_numpy(garbage.view(np.int32).reshape(1, ports, 14, subc).copy()).to(device)
        mod.modulate_slot(g, [(plan, None, 0, cw[:(plan.nof_bits + 7) // 8])])
        if with_csi_rs:
            gen.map_slot(g.view(torch.int16).view(1, ports, 14, subc, 2), [cfg.library()])
        torch.cuda.synchronize()
        return g.cpu().numpy().view(np.uint16).reshape(ports, 14, subc, 2)

    pdsch_only, both, unreserved = run(plan_res, False), run(plan_res, True), run(plan_all, False)
    bits, mask = cm.model_grid([cfg], ports, subc)
    assert mask.sum() == ports * nof_csi_res
    assert np.array_equal(both[mask], bits[mask])
    assert np.array_equal(both[~mask], pdsch_only[~mask])
    assert np.array_equal(pdsch_only[mask], garbage[0][mask])  # the PDSCH kept off the reserved REs
    assert not np.array_equal(pdsch_only, unreserved)
    assert (unreserved[mask] != garbage[0][mask]).any()
    mod.close()


def test_host_form_threads_on_one_handle_keep_their_own_input(gen):
    """Four threads in the host form of ONE generator, each with its own scrambling identity and garbage grid on the
    smallest fixture's resource (tests/host_form_threads.py): every call returns its own thread's grid bit for bit."""
    from tests.host_form_threads import check_isolation

    fx = min(FIXTURES, key=lambda f: (len(f.cfgs), f.nof_grid_ports, f.cfgs[0].nof_rb, f.nof_subc))
    assert fx.name == "row1_one_prb"
    inputs = [(cm.garbage_grid(1, fx.nof_grid_ports, fx.nof_subc, 7000 + i)[0],
               fx.cfgs[0].library(scrambling_id=(fx.cfgs[0].scrambling_id + 1 + 97 * i) % 1024)) for i in range(4)]
    check_isolation(lambda x: gen.map(x[0], x[1]), inputs, lambda grid: grid.tobytes())
