"""PRACH OFDM demodulator on the MI355X (srs_amd_prach_demodulate / srs_amd_prach_demodulate_batch through the Python
layer).

References: the fixtures recorded from the reference's own demodulator (tests/golden/prach_demod_golden.npz, written by
tools/prach_demod_golden_gen.cpp) and the float64 model (tests/prach_demod_model.py).  The GPU is never compared with
itself for accuracy; the batch / stream / padding tests compare outputs of the same deterministic kernels for identity.

Bound, per real component:  |gpu - exact| <= 2^-8 |exact| + A x RMS(exact),  the first term half a bf16 ulp.  A is four
times the largest deviation max |ref - exact| / RMS(exact) of the reference's own recorded output from the model over
all fixtures, 4 x 1.312e-2 = 5.247e-2 (tests/test_prach_demod_model.py prints it; dm.bound_A() recomputes it here): the
GPU is float32 as the reference, with another, equally valid operation order.
Words, against the model: values above 2^-6 x RMS are at most one bf16 word apart, and at most 2e-3 of a fixture's words
differ (the reference itself stays at or below 1e-3, which the CPU test asserts).  Against the fixture the same two with
the triangle inequality: two words, 3e-3.

A demodulator object belongs to one sampling rate, so "every fixture in one call" is one call per sampling rate with
every fixture of that rate: the 30.72 MHz call holds thirteen windows, long and short, planned and split."""
import ctypes
import math

import numpy as np
import pytest

from tests import prach_demod_model as dm
from tests import prach_model as pm

pytestmark = pytest.mark.gpu

ACCEPTED = dm.accepted()
RATES = sorted({fx.srate for fx in ACCEPTED})
A = dm.bound_A()
NAN_WORD = 0x7FC07FC0


def test_bound_is_the_documented_one():
    assert abs(A - 5.247e-2) < 0.0005e-2


@pytest.fixture(scope="module")
def demods(device):
    import srsran_project_amd as amd

    made = {}

    def get(srate):
        if srate not in made:
            made[srate] = amd.PrachDemodulator(srate, device.index or 0)
        return made[srate]

    yield get
    for d in made.values():
        d.close()


_HOST = {}


def _host(demods, fx):
    """The host form's output of a fixture, computed once."""
    if fx.name not in _HOST:
        x, _ = dm.fixture_samples(fx.name)
        out = demods(fx.srate).demodulate(x, fx.config(), nof_samples=fx.nof_samples)
        out.setflags(write=False)
        _HOST[fx.name] = out
    return _HOST[fx.name]


def _check_accuracy(words, exact, model_words, label):
    val = pm.from_cbf16(words)
    e = np.stack([exact.real, exact.imag], axis=-1)
    v = np.stack([val.real, val.imag], axis=-1)
    r = dm.rms(exact)
    excess = np.abs(v - e) - (2.0 ** -8 * np.abs(e) + A * r)
    a, b, c = dm.word_stats(words, exact, model_words)
    print("%s: max |gpu - exact| %.3e x RMS, %.2e of the words differ from the model, distance %d" % (label, a, b, c))
    assert float(excess.max()) <= 0.0, label
    assert c <= 1 and b <= 2e-3, label
    return b


@pytest.mark.parametrize("fx", ACCEPTED, ids=lambda fx: fx.name)
def test_accuracy_host_form(demods, fx):
    out = _host(demods, fx)
    assert out.shape == fx.out.shape
    exact, words = dm.fixture_model(fx.name)
    _check_accuracy(out, exact, words, fx.name)
    # against the reference's recorded output
    dist = np.abs(out.astype(np.int64) - fx.out.astype(np.int64))
    big = np.abs(np.stack([exact.real, exact.imag], axis=-1)) > dm.rms(exact) / 64.0
    print("%s: %.2e of the words differ from the reference's" % (fx.name, float(np.mean(dist != 0))))
    assert int(dist[big].max()) <= 2 and float(np.mean(dist != 0)) <= 3e-3


# ---- batch form -----------------------------------------------------------------------------------------------------

def _batch(dem, device, windows, sample_pads=None, out_pads=None, stream=None):
    """windows: [(config, complex64 [ports, stride], nof_samples)].  Packs the inputs with sample_pads[i] NaN samples
    before window i and NaN beyond nof_samples of every port, the outputs with out_pads[i] NaN words before block i and
    one pad at the end; returns the per-window outputs as uint16 [...] arrays and checks that no pad word was written."""
    import torch

    n = len(windows)
    sample_pads = sample_pads or [0] * n
    out_pads = out_pads or [0] * n
    geos = [dem.geometry(c) for c, _, _ in windows]
    chunks, s_off, pos = [], [], 0
    for (c, x, ns), pad in zip(windows, sample_pads):
        x = np.array(x, np.complex64)
        x[:, ns:] = np.nan
        chunks += [np.full(pad, np.nan, np.complex64), x.reshape(-1)]
        s_off.append(pos + pad)
        pos += pad + x.size
    o_off, opos = [], 0
    for g, pad in zip(geos, out_pads):
        o_off.append(opos + pad)
        opos += pad + g.nof_elements
    total = opos + 3
    samples = torch.from_numpy(np.concatenate(chunks)).to(device)
    out = torch.full((total,), NAN_WORD, dtype=torch.int32, device=device)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(device))
    dem.demodulate_batch(samples, [c for c, _, _ in windows], s_off, [ns for _, _, ns in windows],
                         port_strides=[x.shape[1] for _, x, _ in windows], out=out, out_offsets=o_off, stream=stream)
    (stream or torch.cuda.current_stream(device)).synchronize()
    raw = out.cpu().numpy().view(np.uint32)
    written = np.zeros(total, bool)
    res = []
    for (c, x, _), g, o in zip(windows, geos, o_off):
        written[o:o + g.nof_elements] = True
        w = raw[o:o + g.nof_elements].copy().view(np.uint16)
        res.append(w.reshape(c.nof_td_occasions, c.nof_fd_occasions, c.nof_ports, g.nof_symbols, g.L_ra, 2))
    assert bool((raw[~written] == NAN_WORD).all()), "a pad word was written"
    return res


def _fixture_windows(fxs):
    return [(fx.config(), dm.fixture_samples(fx.name)[0], fx.nof_samples) for fx in fxs]


def _of_rate(srate):
    return [fx for fx in ACCEPTED if fx.srate == srate]


@pytest.mark.parametrize("srate", RATES)
def test_heterogeneous_batch_equals_host_form(demods, device, srate):
    fxs = _of_rate(srate)
    for fx, got in zip(fxs, _batch(demods(srate), device, _fixture_windows(fxs))):
        assert np.array_equal(got, _host(demods, fx)), fx.name


@pytest.mark.parametrize("srate", RATES)
def test_padded_batch_writes_no_pad_word(demods, device, srate):
    fxs = _of_rate(srate)
    spads = [1 + 2 * i for i in range(len(fxs))]            # odd sample offsets
    opads = [(3, 1, 7, 5, 9, 11, 13)[i % 7] for i in range(len(fxs))]  # odd element offsets, odd block starts
    got = _batch(demods(srate), device, _fixture_windows(fxs), spads, opads)
    for fx, g in zip(fxs, got):
        assert np.array_equal(g, _host(demods, fx)), fx.name


def test_non_default_stream(demods, device):
    import torch

    fxs = _of_rate(30720000)
    got = _batch(demods(30720000), device, _fixture_windows(fxs), stream=torch.cuda.Stream(device))
    for fx, g in zip(fxs, got):
        assert np.array_equal(g, _host(demods, fx)), fx.name


def _by_name(*names):
    return [next(f for f in ACCEPTED if f.name == n) for n in names]


@pytest.mark.parametrize("names", [
    ("a1_30.72_mu1_6td", "b4_30.72_mu1"),                 # both 1024 points, planned
    ("f1_15.36", "f2_15.36"),                             # both 12288 points, split
], ids=["planned_1024", "split_12288"])
def test_repeated_dft_size(demods, device, names):
    fxs = _by_name(*names)
    assert fxs[0].ref_geo[2] == fxs[1].ref_geo[2] and fxs[0].format != fxs[1].format
    for fx, g in zip(fxs, _batch(demods(fxs[0].srate), device, _fixture_windows(fxs))):
        assert np.array_equal(g, _host(demods, fx)), fx.name


@pytest.mark.parametrize("names", [
    ("a1_30.72_mu1_6td", "f3_30.72_boost", "a1_30.72_mu2_2fd"),      # 1024, 6144, 512: one launch each, no finish
    ("f0_30.72_mu1_2fd_straddle", "f0_30.72_mu1_slot1"),            # 24576 = 24 x 1024
    ("f0_23.04", "f3_23.04"),                                       # 18 x 1024 and 9 x 512: two sub-transform sizes
], ids=["planned_only", "split_only", "split_two_sub_sizes"])
def test_size_classes(demods, device, names):
    fxs = _by_name(*names)
    planned = [fx.ref_geo[2] in dm.PLANNED for fx in fxs]
    assert all(planned) or not any(planned)
    for fx, g in zip(fxs, _batch(demods(fxs[0].srate), device, _fixture_windows(fxs))):
        assert np.array_equal(g, _host(demods, fx)), fx.name


@pytest.mark.parametrize("name", ["a1_30.72_mu1_6td", "f0_30.72_mu1_slot1"], ids=["planned", "split"])
@pytest.mark.parametrize("ports", [2, 4])
def test_ports(demods, device, name, ports):
    """Every port of a multi-port window, port_stride > nof_samples, equals the one-port call on its own samples."""
    fx = _by_name(name)[0]
    dem = demods(fx.srate)
    stride = fx.nof_samples + 29
    x = dm.generate(fx.seed + 77, ports * stride)[0].reshape(ports, stride)
    got = _batch(dem, device, [(fx.config(nof_ports=ports), x, fx.nof_samples)], [5], [3])[0]
    for p in range(ports):
        alone = dem.demodulate(x[p, :fx.nof_samples], fx.config(nof_ports=1))
        assert np.array_equal(got[:, :, p], alone[:, :, 0]), (name, p)
    exact = dm.exact_output(x[:, :fx.nof_samples], fx.geometry(), fx.nof_td, fx.nof_fd)
    _check_accuracy(got, exact, dm.to_cbf16_once(exact), "%s %d ports" % (name, ports))


# ---- tones ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f0_7.68_straddle_2fd_2ports", "f0_30.72_mu1_2fd_straddle"], ids=["6144", "24576"])
def test_tones(demods, device, name):
    """A window that is zero except for one complex exponential of amplitude 1.5 / sqrt(N) in the DFT window: just
    outside an occasion (subcarriers k_start - 1 and k_start + L_ra) the output is zero up to the float32 transform's
    error, on its first and last subcarrier it is 1.5 in that one bin.  Once for an occasion that straddles the grid
    centre (the fixture's rb_offset) and once for one below it (rb_offset 0).
    Zero bound: a float32 FFT's error is at most about 5 eps log2(N) ||X||_2 (Higham, Accuracy and Stability of
    Numerical Algorithms, Theorem 24.2), ||X||_2 = 1.5 after the scaling, eps = 2^-23."""
    fx = _by_name(name)[0]
    dem = demods(fx.srate)
    windows, expect = [], []
    for rb_offset in (fx.rb_offset, 0):
        cfg = fx.config(rb_offset=rb_offset, nof_ports=1)
        geo = dm.geometry(fx.srate, fx.numerology, fx.slot_index, fx.format, fx.nof_td, fx.nof_fd, fx.start_symbol,
                          rb_offset, fx.nof_prb, 1)
        N, L, k0, half = geo["dft_size"], geo["L_ra"], geo["k_start"][0], geo["grid"] // 2
        assert (k0 < half < k0 + L) == (rb_offset != 0)
        first = geo["sample_offset"][0] + geo["cp_samples"][0]
        for g, inside in ((k0 - 1, None), (k0 + L, None), (k0, 0), (k0 + L - 1, L - 1)):
            x = np.zeros((1, fx.nof_samples), np.complex64)
            n = np.arange(N)
            tone = np.exp(2j * np.pi * ((int(dm.bin_of(g, geo["grid"], N)) * n) % N) / N) * (1.5 / math.sqrt(N))
            x[0, first:first + N] = tone.astype(np.complex64)
            windows.append((cfg, x, fx.nof_samples))
            expect.append(inside)
    N = fx.ref_geo[2]
    zero = 5.0 * 2.0 ** -23 * math.log2(N) * 1.5
    for (cfg, _, _), inside, got in zip(windows, expect, _batch(dem, device, windows)):
        v = pm.from_cbf16(got)  # [1, 2, 1, 1, L]
        want = np.zeros(v.shape, np.complex128)
        if inside is not None:
            want[0, 0, 0, 0, inside] = 1.5
        err = np.abs(v - want)
        print("%s rb_offset %d tone %s: max error %.3e (zero bound %.3e)" % (name, cfg.rb_offset, inside, err.max(), zero))
        assert float(err.max()) <= zero, (name, cfg.rb_offset, inside)
        if inside is not None:
            assert got[0, 0, 0, 0, inside, 0] == 0x3FC0  # 1.5 exactly


# ---- chained with the detector ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["format0", "a1"])
def test_chained_with_the_detector(demods, device, case):
    """Samples -> demodulate_batch -> detect_batch on one stream, no host copy between them: every (td, fd) occasion
    detects its two preambles with their delays, exactly as the detector fed the model's bf16 output does."""
    import torch

    import srsran_project_amd as amd

    srate, ports, nof_fd = 30720000, 2, 2
    if case == "format0":
        fmt, mu, nof_td, prb, rb, ra_scs, zcz, root, thr, margin, ratio = 0, 1, 1, 51, 10, 4, 9, 300, 0.146, 5, 24
        tx = {(0, 0): [(3, 10), (20, 30)], (0, 1): [(7, 22), (41, 5)]}
    else:
        fmt, mu, nof_td, prb, rb, ra_scs, zcz, root, thr, margin, ratio = 4, 1, 2, 51, 4, 1, 8, 60, 0.371, 12, 4
        # preambles of cyclic shift 0 (nine per root): the detector floors the start of the other shifts' windows to a
        # whole IDFT sample, which moves their reported delay by the fraction
        tx = {(0, 0): [(0, 4), (27, 12)], (0, 1): [(9, 9), (54, 3)], (1, 0): [(18, 15), (36, 1)],
              (1, 1): [(45, 6), (63, 13)]}
    geo = dm.geometry(srate, mu, 0, fmt, nof_td, nof_fd, 0, rb, prb, ports)
    dgeo = pm.geometry(fmt, ra_scs, zcz)
    L, ncs = geo["L_ra"], dgeo["N_cs"]
    assert dgeo["idft_size"] * ratio == geo["dft_size"]
    preambles = []
    for (td, fd), lst in tx.items():
        for idx, delay in lst:
            per_root = L // ncs
            u = pm.physical_root(L, root + idx // per_root)
            preambles.append((td, fd, pm.preamble_frequency_domain(L, u, (idx % per_root) * ncs), delay * ratio))
    nof_samples = geo["window_samples"]
    x = dm.transmit(geo, ports, nof_samples, preambles, np.random.default_rng(31), 0.3)

    dem, det = demods(srate), amd.PrachDetector(device.index or 0)
    cfg = amd.PrachDemodConfiguration(format=fmt, numerology=mu, nof_td_occasions=nof_td, nof_fd_occasions=nof_fd,
                                      rb_offset=rb, nof_prb_ul_grid=prb, nof_ports=ports)
    pcfg = amd.PrachConfiguration(format=fmt, ra_scs=ra_scs, root_sequence_index=root, zero_correlation_zone=zcz,
                                  threshold=thr, win_margin=margin, nof_rx_ports=ports)
    pcfgs = [pcfg] * (nof_td * nof_fd)
    stream = torch.cuda.Stream(device)
    samples = torch.from_numpy(x).to(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    out = dem.demodulate_batch(samples, [cfg], [0], [nof_samples], stream=stream)
    raw = det.detect_batch(out, pcfgs, dem.detector_offsets([cfg]), stream=stream)
    stream.synchronize()
    chained = det.results_to_host(raw)

    model_words = dm.to_cbf16_once(dm.exact_output(x, geo, nof_td, nof_fd))  # [td, fd, port, symbol, L, 2]
    for td in range(nof_td):
        for fd in range(nof_fd):
            got = chained[td * nof_fd + fd]
            want = det.detect(model_words[td, fd], pcfg)
            found = [(p.preamble_index, p.delay_samples) for p in got.preambles]
            assert found == sorted(tx[(td, fd)]), (case, td, fd)
            assert found == [(p.preamble_index, p.delay_samples) for p in want.preambles], (case, td, fd)
    det.close()


# ---- invalid calls --------------------------------------------------------------------------------------------------

def test_invalid_calls_launch_nothing(demods, device):
    import torch

    import srsran_project_amd as amd
    from srsran_project_amd import _lib
    from srsran_project_amd.prach_demodulator import _Config, _u64

    fx = _by_name("a1_30.72_mu1_6td")[0]
    dem = demods(fx.srate)
    x, _ = dm.fixture_samples(fx.name)
    good = fx.config(nof_td_occasions=2, nof_fd_occasions=2)
    g = dem.geometry(good)
    samples = torch.from_numpy(np.concatenate([x[0], x[0]])).to(device)
    out = torch.full((2 * g.nof_elements,), NAN_WORD, dtype=torch.int32, device=device)
    n, stride = fx.nof_samples, x.shape[1]

    def call(second, nof=n, port_stride=stride):
        cfgs = (_Config * 2)(good._c(), second._c())
        return dem._lib.srs_amd_prach_demodulate_batch(
            dem._h, cfgs, 2, samples.data_ptr(), _u64([0, stride]), _u64([stride, port_stride]), _u64([n, nof]),
            out.data_ptr(), _u64([0, g.nof_elements]), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))

    bad = [dict(format=14), dict(format=0, numerology=3, nof_td_occasions=1), dict(nof_td_occasions=0),
           dict(format=0, nof_td_occasions=2), dict(nof_fd_occasions=0), dict(nof_fd_occasions=9), dict(nof_ports=0),
           dict(nof_prb_ul_grid=86), dict(rb_offset=28)]
    for over in bad:
        kw = dict(nof_td_occasions=2, nof_fd_occasions=2)
        kw.update(over)
        assert call(fx.config(**kw)) == _lib.SRS_AMD_EINVAL, over
        with pytest.raises(ValueError):
            dem.demodulate(x, fx.config(**kw), nof_samples=n)
    assert call(good, nof=g.min_input_samples - 1) == _lib.SRS_AMD_EINVAL
    assert call(good, port_stride=n - 1) == _lib.SRS_AMD_EINVAL
    with pytest.raises(ValueError):
        dem.demodulate(x[:, :g.min_input_samples - 1], good)
    with pytest.raises(ValueError):
        amd.PrachDemodulator(30720000 + 15000, device.index or 0)  # no plan at this rate
    torch.cuda.synchronize()
    assert bool((out.cpu() == NAN_WORD).all())  # the valid first window was not launched either
    assert call(good) == _lib.SRS_AMD_OK
    torch.cuda.synchronize()
    assert not bool((out.cpu() == NAN_WORD).any())
