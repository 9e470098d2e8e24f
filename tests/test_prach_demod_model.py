"""The PRACH demodulator's float64 model (tests/prach_demod_model.py) and the C-ABI's host-only geometry against the
fixtures recorded from the reference (tests/golden/prach_demod_golden.npz, tools/prach_demod_golden_gen.cpp).  No GPU.

Prints, per fixture, how far the reference's own float32 output is from the model: (a) max |ref - exact| / RMS(exact),
(b) the share of bf16 words that differ from the model's, (c) the largest word distance among values above
2^-6 x RMS.  Four times the largest (a) is the absolute term A of the GPU test's bound."""
import numpy as np
import pytest

from tests import prach_demod_model as dm

FIXTURES = dm.fixtures()
ACCEPTED = dm.accepted()
REJECTED = [fx for fx in FIXTURES if fx.rejected]


def test_fixture_list():
    names = [fx.name for fx in FIXTURES]
    assert len(ACCEPTED) == 23 and len(REJECTED) == 6 and len(set(names)) == len(names)
    assert {fx.ref_geo[2] for fx in ACCEPTED} >= {512, 1024, 4608, 6144, 12288, 18432, 24576, 49152, 98304}


@pytest.mark.parametrize("fx", ACCEPTED, ids=lambda fx: fx.name)
def test_generator_checksum(fx):
    x, checksum = dm.fixture_samples(fx.name)
    assert checksum == fx.checksum
    assert x.shape == (fx.ports, fx.port_stride) and x.dtype == np.complex64


@pytest.mark.parametrize("fx", ACCEPTED, ids=lambda fx: fx.name)
def test_model_geometry_equals_reference(fx):
    g = fx.geometry()
    assert [g["ra_scs"], g["L_ra"], g["dft_size"], g["nof_symbols"], g["window_samples"]] == fx.ref_geo
    assert g["sample_offset"] == list(fx.ref_td[:, 0]) and g["cp_samples"] == list(fx.ref_td[:, 1])
    assert g["k_start"] == fx.ref_k
    assert g["min_input_samples"] <= fx.nof_samples <= fx.port_stride


@pytest.mark.parametrize("fx", ACCEPTED, ids=lambda fx: fx.name)
def test_c_abi_geometry_equals_reference_and_model(fx):
    import srsran_project_amd as amd

    g, m = amd.prach_demod_geometry(fx.srate, fx.config()), fx.geometry()
    assert [g.ra_scs, g.L_ra, g.dft_size, g.nof_symbols, g.window_samples] == fx.ref_geo
    assert g.sample_offset == list(fx.ref_td[:, 0]) and g.cp_samples == list(fx.ref_td[:, 1])
    assert g.k_start == fx.ref_k
    assert g.min_input_samples == m["min_input_samples"] and g.nof_elements == m["nof_elements"] == fx.out.size // 2
    assert g.sub_dft_size * g.nof_sub_dfts == g.dft_size
    assert (g.nof_sub_dfts == 1) == (g.dft_size in dm.PLANNED)
    occasion = fx.ports * g.nof_symbols * g.L_ra
    assert amd.prach_detector_offsets(fx.srate, fx.config(), 5) == [5 + i * occasion
                                                                    for i in range(fx.nof_td * fx.nof_fd)]


@pytest.mark.parametrize("fx", REJECTED, ids=lambda fx: fx.name)
def test_rejected_fixtures_are_invalid(fx):
    import srsran_project_amd as amd

    with pytest.raises(ValueError):
        fx.geometry()
    with pytest.raises(ValueError):
        amd.prach_demod_geometry(fx.srate, fx.config())
    with pytest.raises(ValueError):
        amd.prach_detector_offsets(fx.srate, fx.config())


def _valid():
    fx = next(f for f in ACCEPTED if f.name == "a1_30.72_mu1_6td")
    return fx, dict(format=fx.format, numerology=1, subframe_slot_index=0, nof_td_occasions=2, nof_fd_occasions=2,
                    start_symbol=0, rb_offset=4, nof_prb_ul_grid=51, nof_ports=2)


@pytest.mark.parametrize("srate,over", [
    (30720000, dict(format=14)),
    (30720000, dict(numerology=4)),
    (30720000, dict(subframe_slot_index=2)),
    (30720000, dict(start_symbol=14)),
    (30720000, dict(nof_td_occasions=0)),
    (30720000, dict(nof_td_occasions=8)),
    (30720000, dict(format=0, nof_td_occasions=2)),
    (30720000, dict(nof_fd_occasions=0)),
    (30720000, dict(nof_fd_occasions=9)),
    (30720000, dict(nof_ports=0)),
    (30720000, dict(nof_prb_ul_grid=86)),             # grid 1032 >= dft_size 1024
    (30720000, dict(rb_offset=28)),                   # second occasion ends at subcarrier 12 x 40 + 2 + 139 >= 612
    (122880000, dict(format=0, numerology=3, nof_td_occasions=1)),  # 1.25 kHz with 120 kHz PUSCH: reserved
    (30720000 + 15000, dict()),                       # not 2^a or 3 x 2^a times 15 kHz
    (960000, dict()),                                 # below 1.92 MHz
    (2880000, dict(format=3, numerology=0, nof_td_occasions=1, nof_prb_ul_grid=6, rb_offset=0,
                   nof_fd_occasions=1)),              # 576 points: no plan and no split
], ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else str(v))
def test_invalid_configurations(srate, over):
    import srsran_project_amd as amd

    _, kw = _valid()
    assert amd.prach_demod_geometry(30720000, amd.PrachDemodConfiguration(**kw)).dft_size == 1024
    kw.update(over)
    with pytest.raises(ValueError):
        amd.prach_demod_geometry(srate, amd.PrachDemodConfiguration(**kw))
    m = dict(kw)
    with pytest.raises(ValueError):
        dm.geometry(srate, m["numerology"], m["subframe_slot_index"], m["format"], m["nof_td_occasions"],
                    m["nof_fd_occasions"], m["start_symbol"], m["rb_offset"], m["nof_prb_ul_grid"], m["nof_ports"])


def test_sampling_rate_table():
    """Every rate of ofdm.h with every format family: the C-ABI and the model accept the same ones, with the same
    DFT size and split."""
    import srsran_project_amd as amd

    accepted = 0
    for a in range(8):
        for base in (1920000, 2880000):
            srate = base << a
            for fmt, mu in ((0, 0), (3, 0), (9, 0), (9, 1), (9, 2), (9, 3)):
                prb = {0: 6, 3: 24, 9: 12}[fmt]  # the smallest grid that holds one occasion
                args = (srate, mu, 0, fmt, 1, 1, 0, 0, prb)
                try:
                    m = dm.geometry(*args)
                except ValueError:
                    m = None
                cfg = amd.PrachDemodConfiguration(format=fmt, numerology=mu, nof_prb_ul_grid=prb)
                if m is None:
                    with pytest.raises(ValueError):
                        amd.prach_demod_geometry(srate, cfg)
                    continue
                g = amd.prach_demod_geometry(srate, cfg)
                accepted += 1
                assert g.dft_size == m["dft_size"] and g.cp_samples == m["cp_samples"]
                if g.dft_size not in dm.PLANNED:
                    assert g.sub_dft_size == next(s for s in (1024, 512, 256) if g.dft_size % s == 0)
    assert accepted >= 56, accepted


def test_reference_deviation_from_the_model():
    """The reference's own distance from the model: printed per fixture; its word share stays at or below 1e-3 (the
    generator keeps only such seeds).  The generator measured it against direct sums, this model uses numpy.fft: a bin
    whose exact value is a bf16 tie (the samples are multiples of 1 / 128, so bins with trivial twiddles can be) falls
    to either side in the two float64 evaluations, hence one word of slack between the two shares."""
    rows = dm.reference_deviation()
    for (name, a, b, c), fx in zip(rows, ACCEPTED):
        print("%-30s N %6d  (a) %.3e x RMS  (b) %.2e of the words  (c) %d" % (name, fx.ref_geo[2], a, b, c))
        assert b <= 1e-3 and c <= 1, name
        assert abs(b - fx.ref_share) * fx.out.size <= 1.0 + 1e-9, name
    print("A = 4 x max (a) = %.3e" % dm.bound_A())
    # (a) is dominated by the bf16 rounding itself, half a bf16 ulp of the largest values: a few 2^-9 of the RMS
    assert 2.0 ** -9 < dm.bound_A() / 4.0 < 2.0 ** -5


def test_single_rounding():
    """to_bf16_once rounds once: a double just above a bf16 tie goes up although its float32 image is the tie."""
    tie = np.float64(1.0 + 2.0 ** -8)
    assert list(dm.to_bf16_once(np.array([tie, tie + 2.0 ** -40, tie - 2.0 ** -40, 1.0 + 3 * 2.0 ** -8]))) == [
        0x3F80, 0x3F81, 0x3F80, 0x3F82]
