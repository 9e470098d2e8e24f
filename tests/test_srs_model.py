"""SRS channel estimator, CPU side (no GPU, no reference tree).

* the float64 model (tests/srs_model.py) reproduces every fixture of tests/golden/srs_golden.npz -- the reference's
  own estimator run by tools/srs_golden_gen.cpp: the integer correlation peak, the time-alignment range and
  resolution, the class of every field on the all-zero grid, and the float fields within the bounds below;
* the library's host srs_information equals the ~500 resources the generator recorded from get_srs_information, and
  its bandwidth table all 256 pairs recorded from srs_configuration_get, exactly;
* every invalid configuration returns SRS_AMD_EINVAL (ValueError) from the host-only functions and from the
  validation the estimate calls use;
* the fixtures are well conditioned: the integer peak stands clear of every sample of the search ranges more than
  two taps away.

Bounds of the model-vs-reference comparison, from the number formats and not from either result.  The reference is
float32 throughout.  A wideband coefficient is a mean of M <= 1632 float32 products: about eps sqrt(M) = 2.4e-6
relative.  On top of that the phase-table index is a rounded float32 quantity: an element whose index lands within
rounding of a half-integer may take the neighbouring entry in one implementation and not in the other, which turns
that element by 2 pi / 1024 and the coefficient by at most 6.2e-3 / M of the element; a handful of such elements
stay below 1e-4 of the matrix norm.  noise_variance is a sum of squared residuals; where the residual is only the
bf16 rounding of the grid (the noiseless fixture) it is 1e-5 of the signal and the float32 rounding of the signal
terms shows as about eps / 1e-5^(1/2) per element: 1e-3 relative covers it.  The powers in dB are 10 log10 of sums
of positive terms, 4.3 x the relative error plus half an ulp of the dB value: 1e-4 dB with the index effect.  The
fractional tap is a ratio of weighted sums of five float32 correlation samples, each good to about eps log2(N): 1e-5
samples.  The deviations actually measured are printed and written in DESIGN.md; the GPU bound derives from them
(tests/test_srs_gpu.py).
"""
import math

import numpy as np
import pytest

from tests import srs_model as sm

FIXTURES = sm.fixtures()
IDS = [fx.name for fx in FIXTURES]
T_C = sm.T_C
DBL_MIN = 2.2250738585072014e-308


def _value_class(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("+inf" if v > 0 else "-inf") if math.isinf(v) else "finite"


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_model_reproduces_reference(fx):
    m = fx.model()
    assert abs(m["ta_resolution_s"] - fx.ta_resolution_s) < 0.5 * T_C
    assert abs(m["ta_max_s"] - fx.ta_max_s) < 0.5 * T_C
    # the quirk srs.h describes: the reference's combined minimum is the smallest positive double
    assert fx.ta_min_s == DBL_MIN
    if fx.all_zero:
        got = [m["matrix"].real, m["matrix"].imag, m["epre_db"], m["rsrp_db"], m["noise_variance"], m["time_alignment_s"]]
        ref = [fx.matrix.real, fx.matrix.imag, fx.epre_db, fx.rsrp_db, fx.noise_variance, fx.time_alignment_s]
        for g, r in zip(got, ref):
            assert [_value_class(v) for v in np.ravel(g)] == [_value_class(v) for v in np.ravel(r)]
        return
    if fx.cfg.nof_antenna_ports == 1:  # the mean over one port is the port's own measurement
        assert round(fx.time_alignment_s / fx.ta_resolution_s) == m["idx_ports"][0]
    coef = np.abs(fx.matrix - m["matrix"]).max() / np.linalg.norm(m["matrix"])
    nv = abs(float(fx.noise_variance) - m["noise_variance"]) / m["noise_variance"]
    epre, rsrp = abs(float(fx.epre_db) - m["epre_db"]), abs(float(fx.rsrp_db) - m["rsrp_db"])
    ta = abs(fx.time_alignment_s - m["time_alignment_s"]) / m["ta_resolution_s"]
    print("%s: reference vs model: coefficients %.3e of the norm, noise variance %.3e relative, epre %.3e dB, rsrp %.3e dB,"
          " time alignment %.3e samples" % (fx.name, coef, nv, epre, rsrp, ta))
    assert coef < 1e-4 and nv < 1e-3 and epre < 1e-4 and rsrp < 1e-4 and ta < 1e-5
    # the delay the generator applied is what the estimator measures, to a fraction of a tap
    assert abs(m["time_alignment_s"] - fx.delay_s) < 0.5 * m["ta_resolution_s"]


def test_reference_deviation_is_reported():
    dev = sm.reference_deviation()
    print("reference vs float64 model: coefficients %.3e of the norm, noise variance %.3e relative, epre %.3e dB, "
          "rsrp %.3e dB, time alignment %.3e samples" % dev)
    assert dev[0] < 1e-4 and dev[1] < 1e-3 and dev[2] < 1e-4 and dev[3] < 1e-4 and dev[4] < 1e-5


def test_fixtures_cover_the_listed_shapes():
    cfgs = [fx.cfg for fx in FIXTURES]
    lengths = {sm.information(c, 0)[0] for c in cfgs}
    assert {12, 24, 144, 156, 408, 816, 1632} <= lengths
    assert {sm.idft_size(M) for M in lengths} == {128, 256, 512, 1024, 2048}
    assert {c.nof_antenna_ports for c in cfgs} == {1, 2, 4} and {c.nof_symbols for c in cfgs} == {1, 2, 4}
    assert {len(c.rx_ports) for c in cfgs} >= {1, 2, 4} and any(c.rx_ports == [2, 0] for c in cfgs)
    for comb in (2, 4):
        four = [c for c in cfgs if c.nof_antenna_ports == 4 and c.comb_size == comb]
        half = (12 if comb == 4 else 8) // 2
        assert any(c.cyclic_shift < half for c in four) and any(c.cyclic_shift >= half for c in four)
    assert any(c.start_symbol + c.nof_symbols == 14 and c.nof_symbols > 1 for c in cfgs)
    assert any(c.bandwidth_index > 0 and c.freq_position > 0 and c.freq_shift > 0 for c in cfgs)
    assert {c.numerology for c in cfgs} == {0, 1}
    delays = [fx.delay_s for fx in FIXTURES if not fx.all_zero]
    assert min(delays) < 0 < max(delays) and 0.0 in delays
    assert sum(fx.all_zero for fx in FIXTURES) == 1
    # the 40 dB clamp branch: a fixture whose noise variance is below 1e-4 of the RSRP
    assert any(not fx.all_zero and float(fx.noise_variance) < 1e-4 * 10 ** (float(fx.rsrp_db) / 10) for fx in FIXTURES)


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixtures_are_well_conditioned(fx):
    """The integer peak exceeds every sample more than two taps away inside the two search ranges by a factor of 1.5.
    A sequence of M elements in an N-point transform has a main lobe of N / M taps; for M = 12 (N = 128) that is 10.7
    taps, wider than the whole search range, and the sample three taps from the peak is sinc^2(3 x 12 / 128) = 0.766
    of it whatever the seed: the factor cannot exceed 1.31 there.  Such a fixture is held to 0.9 of its own ceiling."""
    if fx.all_zero:
        return
    m = fx.model()
    M, N = sm.information(fx.cfg, 0)[0], m["idft_size"]
    ceiling = 1.0 / np.sinc(3.0 * M / N) ** 2
    margin = sm.peak_margin(m)
    print("%s: peak over the far samples %.2f (main-lobe ceiling %.2f)" % (fx.name, margin, ceiling))
    assert margin >= (1.5 if ceiling >= 1.5 / 0.9 else 0.9 * ceiling)
    assert ceiling >= 1.5 / 0.9 or M == 12


def test_information_matches_the_recorded_resources():
    import srsran_project_amd as amd

    z = sm.golden()
    assert z["info_in"].shape[0] >= 480
    for row, want in zip(z["info_in"], z["info_out"]):
        nap, c_srs, seq_id, b_srs, comb, offset, cs, n_rrc, n_shift, ap = (int(v) for v in row)
        kw = dict(nof_antenna_ports=nap, nof_symbols=1, start_symbol=0, configuration_index=c_srs, sequence_id=seq_id,
                  bandwidth_index=b_srs, comb_size=comb, comb_offset=offset, cyclic_shift=cs, freq_position=n_rrc,
                  freq_shift=n_shift, freq_hopping=3)
        info = amd.srs_information(amd.SrsConfiguration(**kw), ap)
        got = [info.sequence_length, info.sequence_group, info.sequence_number, info.n_cs, info.n_cs_max,
               info.mapping_initial_subcarrier, info.comb_size]
        assert got == [int(v) for v in want], row
        assert info.idft_size == sm.idft_size(info.sequence_length)
        assert list(sm.information(sm.Config(**kw), ap)) == got  # the model's own restatement


def test_bandwidth_table_matches_the_recorded_pairs():
    import srsran_project_amd as amd

    t = sm.golden()["bandwidth"]
    assert t.shape == (64, 4, 2)
    for c_srs in range(64):
        for b_srs in range(4):
            assert amd.srs_bandwidth(c_srs, b_srs) == (int(t[c_srs, b_srs, 0]), int(t[c_srs, b_srs, 1]))
    for bad in ((64, 0), (0, 4), (255, 255)):
        with pytest.raises(ValueError):
            amd.srs_bandwidth(*bad)


INVALID = [
    ("comb offset >= comb size", dict(comb_size=2, comb_offset=2, cyclic_shift=0)),
    ("comb offset >= comb size (4)", dict(comb_offset=4)),
    ("cyclic shift > 7 with comb 2", dict(comb_size=2, comb_offset=0, cyclic_shift=8)),
    ("cyclic shift > 11 with comb 4", dict(cyclic_shift=12)),
    ("invalid c_srs", dict(configuration_index=64)),
    ("invalid b_srs", dict(bandwidth_index=4, freq_hopping=3)),
    ("frequency hopping", dict(bandwidth_index=2, freq_hopping=1)),
    ("group hopping", dict(hopping=1)),
    ("sequence hopping", dict(hopping=2)),
    ("3 antenna ports", dict(nof_antenna_ports=3)),
    ("0 antenna ports", dict(nof_antenna_ports=0)),
    ("3 symbols", dict(nof_symbols=3)),
    ("8 symbols", dict(nof_symbols=8, start_symbol=0)),
    ("start + symbols > 14", dict(start_symbol=11, nof_symbols=4)),
    ("start symbol 14", dict(start_symbol=14, nof_symbols=1)),
    ("comb 3", dict(comb_size=3, comb_offset=0)),
]
INVALID_GRID = [
    ("empty rx port list", dict(rx_ports=[])),
    ("five rx ports", dict(rx_ports=[0, 1, 2, 3, 0])),
    ("port outside the grid", dict(rx_ports=[0, 4])),
    ("last RE outside nof_subc", dict(freq_shift=1)),
]


def _valid(**over):
    import srsran_project_amd as amd

    # m_SRS = 48, comb 4: M = 144, the last RE is subcarrier 3 + 4 x 143 = 575 of a 576-subcarrier grid
    kw = dict(nof_antenna_ports=2, nof_symbols=2, start_symbol=12, configuration_index=12, sequence_id=5,
              bandwidth_index=0, comb_size=4, comb_offset=3, cyclic_shift=1, freq_position=0, freq_shift=0,
              freq_hopping=0, rx_ports=[0, 3])
    kw.update(over)
    return amd.SrsConfiguration(**kw)


def test_valid_configuration_is_accepted():
    import srsran_project_amd as amd

    assert amd.srs_information(_valid(), 1).sequence_length == 144
    amd.srs_validate(_valid(), 4, 576)
    with pytest.raises(ValueError):
        amd.srs_information(_valid(), 2)  # antenna port outside the resource


@pytest.mark.parametrize("name,bad", INVALID, ids=[n for n, _ in INVALID])
def test_invalid_resource_is_rejected(name, bad):
    import srsran_project_amd as amd

    with pytest.raises(ValueError):
        amd.srs_information(_valid(**bad), 0)
    with pytest.raises(ValueError):
        amd.srs_validate(_valid(**bad), 4, 3300)


@pytest.mark.parametrize("name,bad", INVALID_GRID, ids=[n for n, _ in INVALID_GRID])
def test_invalid_ports_or_grid_are_rejected(name, bad):
    import srsran_project_amd as amd

    with pytest.raises(ValueError):
        amd.srs_validate(_valid(**bad), 4, 576)
