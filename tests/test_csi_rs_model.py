"""NZP-CSI-RS on the host: the numpy model of tests/csi_rs_model.py against the grids recorded from the reference's
own generator (tests/golden/csi_rs_golden.npz, written by tools/csi_rs_golden_gen.cpp), and the host-only entry points
of include/srsran_amd/csi_rs.h (pattern, reserved REs, validation) against the recorded patterns and the model.

The model is float64 rounded once to bf16; the reference is float32 rounded to bf16.  Where every CSI-RS port has one
non-zero weight each transmit port receives a single product, the two agree bit for bit (the sign of a zero included);
with full weight matrices the float32 sums may round to the neighbouring bf16, so those are held to one bf16 ulp.
"""
import numpy as np
import pytest

from tests import csi_rs_model as cm

FIXTURES = cm.fixtures()
IDS = [fx.name for fx in FIXTURES]


def _amd():
    import srsran_project_amd as amd

    return amd


def test_every_listed_case_is_recorded():
    assert len(FIXTURES) == 18
    z = cm.golden()
    assert z["pattern_in"].shape == (300, 14) and z["pattern_out"].shape == (300, 36)
    assert z["ref_map_us"].shape == (2,) and (z["ref_map_us"] > 0).all()
    rows = sorted({c.row for fx in FIXTURES for c in fx.cfgs})
    assert rows == [1, 2, 3, 4, 5]
    # the "generic" precoder list is expected to be empty or nearly so
    assert sum(len(fx.gen_idx) for fx in FIXTURES) <= 8


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_model_equals_reference(fx):
    bits, mask = fx.model()
    ref = fx.reference()
    # the reference wrote nothing outside the model's REs (the grid was zeroed), and only the stored symbol rows
    assert not ref[~mask].any()
    assert sorted(set(np.nonzero(mask)[1].tolist())) == fx.symbols
    if all(cm.one_nonzero_weight_per_port(c) for c in fx.cfgs):
        assert np.array_equal(bits[mask], ref[mask])
    else:
        d = cm.bf16_ulp_distance(bits[mask], ref[mask])
        print("%s: %d of %d halves differ by one bf16 ulp" % (fx.name, int((d == 1).sum()), d.size))
        assert d.max() <= 1
        # a float32 sum is within ~2^-23 relative of the exact one and bf16 values lie 2^-8 apart, so only a value
        # that close to a rounding tie can land on the neighbour: a tiny fraction.  0.9 is a loose floor against a
        # model that is systematically one ulp off, not a measured figure.
        assert (d == 0).mean() > 0.9


def test_c_init_is_the_wrapped_32_bit_value():
    for mu, slot, l, n_id in [(3, 79, 13, 1023), (3, 79, 0, 1023), (1, 19, 13, 1023), (0, 0, 0, 0), (4, 159, 13, 1023)]:
        cfg = cm.Config(row=1, k_ref=[0], symbol_l0=l, start_rb=0, nof_rb=1, freq_density=cm.D_THREE, numerology=mu,
                        slot_index=slot, scrambling_id=n_id)
        wrapped = (((1024 * (14 * slot + l + 1)) % 2 ** 32) * (2 * n_id + 1) % 2 ** 32 + n_id) % 2 ** 32 % 2 ** 31
        assert cm.c_init(cfg, l) == wrapped
    # the case of the fixture does pass 2^31
    assert 1024 * (14 * 79 + 13 + 1) * (2 * 1023 + 1) > 2 ** 31


def _lib_pattern(cfg):
    p = _amd().csi_rs_pattern(cfg.library())
    return [p.rb_begin, p.rb_end, p.rb_stride, p.nof_ports], list(zip(p.re_masks, p.symbol_masks))


def test_pattern_equals_the_recorded_300():
    z = cm.golden()
    rows_seen = set()
    for pin, pout in zip(z["pattern_in"], z["pattern_out"]):
        cfg = cm.pattern_config(pin)
        rows_seen.add(cfg.row)
        head, ports = _lib_pattern(cfg)
        n = int(pout[3])
        want = [(int(pout[4 + 2 * q]), int(pout[5 + 2 * q])) for q in range(n)]
        assert head == [int(v) for v in pout[:4]], pin
        assert ports == want, pin
        # and the model's reading of Table 7.4.1.5.3-1
        rbs, mports = cm.pattern(cfg)
        assert mports == want, pin
        assert rbs == list(range(head[0], head[1], head[2])), pin
    assert rows_seen == set(range(1, 13))


def _reserved_res(cfg):
    out = set()
    pats = _amd().csi_rs_reserved(cfg.library())
    assert 1 <= len(pats) <= 8
    for r in pats:
        for n in r.crbs:
            for k in range(12):
                if (r.re_mask >> k) & 1:
                    out.update((l, 12 * n + k) for l in range(14) if (r.symbols >> l) & 1)
    return out, pats


def test_reserved_is_the_union_of_the_pattern():
    z = cm.golden()
    cfgs = [c for fx in FIXTURES for c in fx.cfgs] + [cm.pattern_config(p) for p in z["pattern_in"]]
    for cfg in cfgs:
        got, pats = _reserved_res(cfg)
        assert got == cm.pattern_res(cfg), cfg
        # one entry per CDM group with distinct REs
        keys = [(r.re_mask, r.symbols) for r in pats]
        assert len(keys) == len(set(keys)) == len(set(cm.pattern(cfg)[1]))
    # ready for the PDSCH modulator's configuration
    amd = _amd()
    pats = amd.csi_rs_reserved(FIXTURES[0].cfgs[0].library())
    mod = amd.PdschModulatorConfig(rnti=1, bwp_start=0, bwp_size=52, modulation=2, crbs=list(range(52)), start_symbol=2,
                                   nof_symbols=12, dmrs_symb_pos=1 << 2, reserved=pats)
    assert mod._c().nof_reserved == len(pats)


def _base(**over):
    kw = dict(row=3, k_ref=[4], symbol_l0=5, start_rb=2, nof_rb=20, cdm=cm.CDM_FD2, freq_density=cm.D_ONE,
              scrambling_id=10, numerology=1, slot_index=3)
    kw.update(over)
    return cm.Config(**kw)


INVALID_PATTERN = {
    "row_0": _base(row=0),
    "row_13": _base(row=13),
    "row_19": _base(row=19),
    "k_ref_count": _base(k_ref=[4, 5]),
    "k_ref_count_row6": _base(row=6, k_ref=[0, 2, 4]),
    "k_ref_range_row1": _base(row=1, k_ref=[4], cdm=cm.CDM_NONE, freq_density=cm.D_THREE),
    "k_ref_range_row2": _base(row=2, k_ref=[12], cdm=cm.CDM_NONE),
    "k_ref_range_row3": _base(k_ref=[11]),
    "k_ref_range_row4": _base(row=4, k_ref=[9]),
    "k_ref_range_row8": _base(row=8, k_ref=[0, 11], cdm=cm.CDM_FD2_TD2),
    "density_row1": _base(row=1, k_ref=[0], cdm=cm.CDM_NONE, freq_density=cm.D_ONE),
    "density_row3_three": _base(freq_density=cm.D_THREE),
    "density_row4_dot5": _base(row=4, freq_density=cm.D_EVEN),
    "density_unknown": _base(freq_density=4),
    "cdm_row1": _base(row=1, k_ref=[0], cdm=cm.CDM_FD2, freq_density=cm.D_THREE),
    "cdm_row3_none": _base(cdm=cm.CDM_NONE),
    "cdm_row8_fd2": _base(row=8, k_ref=[0, 2], cdm=cm.CDM_FD2),
    "cdm8_row12": _base(row=12, k_ref=[0, 2, 4, 6], cdm=cm.CDM_FD2_TD4),
    "symbol_14": _base(symbol_l0=14),
    "symbol_row5_l0_13": _base(row=5, symbol_l0=13),
    "symbol_row8_l0_13": _base(row=8, k_ref=[0, 2], cdm=cm.CDM_FD2_TD2, symbol_l0=13),
    "symbol_row11_l0_13": _base(row=11, k_ref=[0, 2, 4, 6], symbol_l0=13),
}


@pytest.mark.parametrize("name", sorted(INVALID_PATTERN))
def test_invalid_pattern_is_rejected(name):
    amd = _amd()
    cfg = INVALID_PATTERN[name].library()
    for call in (lambda: amd.csi_rs_pattern(cfg), lambda: amd.csi_rs_reserved(cfg),
                 lambda: amd.csi_rs_validate(cfg, 4, 3276)):
        with pytest.raises(ValueError):
            call()


INVALID_MAP = {
    "row_6": (_base(row=6, k_ref=[0, 2, 4, 6]), 4, 3276),
    "row_8": (_base(row=8, k_ref=[0, 2], cdm=cm.CDM_FD2_TD2), 4, 3276),
    "row_12": (_base(row=12, k_ref=[0, 2, 4, 6], cdm=cm.CDM_FD2_TD2), 4, 3276),
    "ports_beyond_grid": (_base(), 1, 3276),
    "ports_beyond_grid_row4": (_base(row=4), 2, 3276),
    "beyond_subcarriers": (_base(start_rb=2, nof_rb=20), 4, 22 * 12 - 1),
    "nof_rb_0": (_base(nof_rb=0), 4, 3276),
    "dot5_even_on_one_odd_prb": (_base(freq_density=cm.D_EVEN, start_rb=3, nof_rb=1), 4, 3276),
    "dot5_odd_on_one_even_prb": (_base(row=2, cdm=cm.CDM_NONE, freq_density=cm.D_ODD, start_rb=4, nof_rb=1), 4, 3276),
    "scrambling_id_1024": (_base(scrambling_id=1024), 4, 3276),
    "slot_beyond_frame": (_base(numerology=1, slot_index=20), 4, 3276),
    "slot_beyond_frame_mu3": (_base(numerology=3, slot_index=80), 4, 3276),
    "numerology_5": (_base(numerology=5, slot_index=0), 4, 3276),
}


@pytest.mark.parametrize("name", sorted(INVALID_MAP))
def test_invalid_mapping_is_rejected(name):
    cfg, ports, subc = INVALID_MAP[name]
    with pytest.raises(ValueError):
        _amd().csi_rs_validate(cfg.library(), ports, subc)


def test_row_8_has_a_pattern_but_cannot_be_mapped():
    amd = _amd()
    cfg = _base(row=8, k_ref=[0, 6], cdm=cm.CDM_FD2_TD2).library()
    p = amd.csi_rs_pattern(cfg)
    assert p.nof_ports == 8 and p.symbol_masks[0] == 0b11 << 5 and p.re_masks[4] == 0b11 << 6
    assert len(amd.csi_rs_reserved(cfg)) == 2
    with pytest.raises(ValueError, match="rows 1 to 5"):
        amd.csi_rs_validate(cfg, 8, 3276)


def test_valid_configurations_pass_validation():
    amd = _amd()
    for fx in FIXTURES:
        for c in fx.cfgs:
            amd.csi_rs_validate(c.library(), fx.nof_grid_ports, fx.nof_subc)
    amd.csi_rs_validate(_base(numerology=3, slot_index=79).library(), 2, 22 * 12)
