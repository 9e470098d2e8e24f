"""PRACH detector on the MI355X (srs_amd_prach_detect / srs_amd_prach_detect_batch through the Python layer).

References: the fixtures recorded from the reference's own detector (tests/golden/prach_golden.npz, written by
tools/prach_golden_gen.cpp) and the float64 model (tests/prach_model.py).  The GPU is never compared with itself
for accuracy; the batch / stream tests compare raw results of the same deterministic kernels for identity.

Exact: the detected preamble indices and their order, delay_samples, nof_detected, the NaN / -1 entries outside the
requested range.  Times: within half a T_c.

Tolerances of the float fields.  Measured on the fixtures, the reference (float32) deviates from the float64 model by
at most
    detection_metric   2.32e-4 relative   (den is a difference of nearly equal sums: the error grows with the metric)
    preamble_power_db  1.27e-6 dB
    rssi_db            9.92e-7 dB
(tests/test_prach_model.py prints them; pm.reference_deviation() recomputes them here).  The GPU is float32 too, with
another, equally valid DFT ordering, and gets four times that: 9.3e-4 relative, 5.1e-6 dB, 4.0e-6 dB, against the
fixtures and against the model.
"""
import math

import numpy as np
import pytest

from tests import prach_model as pm

pytestmark = pytest.mark.gpu

FIXTURES = pm.fixtures()
IDS = [fx.name for fx in FIXTURES]
T_C = pm.T_C
_DEV = pm.reference_deviation()
TOL_METRIC, TOL_POWER_DB, TOL_RSSI_DB = (4.0 * float(v) for v in _DEV)


def test_tolerances_are_the_documented_ones():
    assert abs(TOL_METRIC - 9.3e-4) < 0.05e-4 and abs(TOL_POWER_DB - 5.1e-6) < 0.05e-6 and abs(TOL_RSSI_DB - 4.0e-6) < 0.05e-6


@pytest.fixture(scope="module")
def detector(device):
    import srsran_project_amd as amd

    det = amd.PrachDetector(device.index or 0)
    yield det
    det.close()


def _config(fx, **over):
    import srsran_project_amd as amd

    kw = dict(format=fx.format, ra_scs=fx.ra_scs, root_sequence_index=fx.root_sequence_index,
              zero_correlation_zone=fx.zcz, threshold=fx.threshold, win_margin=fx.win_margin, nof_rx_ports=fx.ports,
              start_preamble_index=fx.start, nof_preamble_indices=fx.nof, combine_symbols=fx.combine,
              idft_size=fx.idft_size)
    kw.update(over)
    return amd.PrachConfiguration(**kw)


def _check_against_model(res, m, start, end, label):
    """res: PrachDetectionResult of the GPU; m: the float64 model's dict."""
    assert [(p.preamble_index, p.delay_samples) for p in res.preambles] == [(d[0], d[1]) for d in m["detected"]], label
    assert abs(res.time_resolution_s - m["time_resolution_s"]) < 0.5 * T_C
    assert abs(res.time_advance_max_s - m["time_advance_max_s"]) < 0.5 * T_C
    if math.isinf(m["rssi_db"]):
        assert res.rssi_db == m["rssi_db"]
    else:
        print("%s rssi %.3e dB from the model" % (label, abs(res.rssi_db - m["rssi_db"])))
        assert abs(res.rssi_db - m["rssi_db"]) <= TOL_RSSI_DB, label
    for p, d in zip(res.preambles, m["detected"]):
        print("%s preamble %d: metric %.3e relative, power %.3e dB from the model" % (
            label, p.preamble_index, abs(p.detection_metric - d[3]) / d[3], abs(p.preamble_power_db - d[4])))
        assert abs(p.time_advance_s - d[2]) < 0.5 * T_C
        assert abs(p.detection_metric - d[3]) <= TOL_METRIC * d[3], label
        assert abs(p.preamble_power_db - d[4]) <= TOL_POWER_DB, label
        assert res.delay_samples[p.preamble_index] == p.delay_samples
        assert res.peak_over_threshold[p.preamble_index] == np.float32(p.detection_metric)
    pot = m["peak_over_threshold"]
    for i in range(64):
        if start <= i < end and not np.isnan(pot[i]):
            assert abs(res.peak_over_threshold[i] - pot[i]) <= TOL_METRIC * pot[i], (label, i)
            assert 0 <= res.delay_samples[i]
        else:
            assert np.isnan(res.peak_over_threshold[i]) and res.delay_samples[i] == -1, (label, i)


def _check_fixture(res, fx):
    ref = [(int(d[0]), int(round(d[1] / fx.time_resolution_s))) for d in fx.det]
    assert [(p.preamble_index, p.delay_samples) for p in res.preambles] == ref, fx.name
    assert abs(res.time_resolution_s - fx.time_resolution_s) < 0.5 * T_C
    assert abs(res.time_advance_max_s - fx.time_advance_max_s) < 0.5 * T_C
    if math.isinf(fx.rssi_db):
        assert res.rssi_db == fx.rssi_db
    else:
        print("%s rssi %.3e dB from the reference" % (fx.name, abs(res.rssi_db - fx.rssi_db)))
        assert abs(res.rssi_db - fx.rssi_db) <= TOL_RSSI_DB
    for p, r in zip(res.preambles, fx.det):
        print("%s preamble %d: metric %.3e relative, power %.3e dB from the reference" % (
            fx.name, p.preamble_index, abs(p.detection_metric - r[2]) / r[2], abs(p.preamble_power_db - r[3])))
        assert abs(p.time_advance_s - r[1]) < 0.5 * T_C
        assert abs(p.detection_metric - r[2]) <= TOL_METRIC * r[2]
        assert abs(p.preamble_power_db - r[3]) <= TOL_POWER_DB
    _check_against_model(res, pm.model_of(fx), 0 if math.isinf(fx.rssi_db) else fx.start,
                         0 if math.isinf(fx.rssi_db) else fx.start + fx.nof, fx.name)
    # an undetected window at the threshold would make the set comparison ill-conditioned: such a fixture's seed is
    # replaced in tools/prach_golden_gen.cpp instead
    detected = {p.preamble_index for p in res.preambles}
    assert all(not res.peak_over_threshold[i] > 0.98 for i in range(64) if i not in detected), fx.name


def _pack(blocks, pads, device):
    """uint16 [.., 2] blocks -> one device buffer with `pads[i]` unused cbf16 elements before block i; offsets in
    cbf16 elements."""
    import torch

    parts, offsets, pos = [], [], 0
    for b, pad in zip(blocks, pads):
        parts.append(np.full((pad, 2), 0x7FC0, np.uint16))  # bf16 NaN: reading a pad shows up
        pos += pad
        offsets.append(pos)
        parts.append(np.ascontiguousarray(b, np.uint16).reshape(-1, 2))
        pos += parts[-1].shape[0]
    buf = np.concatenate(parts).view(np.int16)
    return torch.from_numpy(buf).to(device), offsets


@pytest.mark.parametrize("fx", FIXTURES, ids=IDS)
def test_fixture_host_form(detector, fx):
    _check_fixture(detector.detect(fx.x, _config(fx)), fx)


def test_fixtures_one_heterogeneous_batch(detector, device):
    import torch

    sym, offsets = _pack([fx.x for fx in FIXTURES], [0] * len(FIXTURES), device)
    raw = detector.detect_batch(sym, [_config(fx) for fx in FIXTURES], offsets)
    torch.cuda.synchronize()
    for res, fx in zip(detector.results_to_host(raw), FIXTURES):
        _check_fixture(res, fx)


# ---- fresh seeded inputs against the float64 model ---------------------------------------------------------------

class Fresh:
    def __init__(self, name, fmt, scs, zcz, root, ports, preambles, threshold, margin, start=0, nof=64, combine=True,
                 idft_size=0, sigma=1.0, seed=0):
        self.name, self.format, self.ra_scs, self.zcz, self.root_sequence_index = name, fmt, scs, zcz, root
        self.ports, self.threshold, self.win_margin, self.start, self.nof = ports, threshold, margin, start, nof
        self.combine, self.idft_size = combine, idft_size
        g = pm.geometry(fmt, scs, zcz, idft_size)
        self.idft_size = g["idft_size"]
        limit = 0.8 * g["max_delay_samples"]
        self.tx = [(i, int(f * limit)) for i, f in preambles]
        self.x = pm.make_occasion(np.random.default_rng(seed), fmt, scs, zcz, root, ports, self.tx, sigma, idft_size)
        self._model = None

    def model(self):
        if self._model is None:
            self._model = pm.detect(pm.from_cbf16(self.x), self.format, self.ra_scs, self.zcz,
                                    self.root_sequence_index, self.start, self.nof, self.threshold, self.win_margin,
                                    self.combine, self.idft_size)
        return self._model


_fresh = None


def fresh_cases():
    """Shapes the fixtures do not hold: other roots, 3 ports, the 512- and 2048-point kernels (the latter with two
    wavefronts per workgroup), a format outside the reference's threshold table (C2), B1 and A3 without symbol
    combination, a range that ends inside a root.  Built once."""
    global _fresh
    if _fresh is None:
        _fresh = [
            Fresh("f0_zcz4_3ports", 0, 4, 4, 611, 3, [(37, 0.5), (38, 0.2)], 0.2, 5, seed=1),
            Fresh("f2_zcz10_3ports_2048", 2, 4, 10, 837, 3, [(11, 0.6), (63, 0.3)], 0.12, 9, idft_size=2048, seed=2),
            Fresh("f3_zcz13_1port_2048_range", 3, 5, 13, 222, 1, [(5, 0.4), (2, 0.7)], 0.3, 6, start=3, nof=6,
                  idft_size=2048, seed=3),
            Fresh("c2_15khz_zcz12_3ports", 10, 0, 12, 136, 3, [(0, 0.1), (44, 0.9)], 0.25, 12, seed=4),
            Fresh("b1_60khz_zcz6_3ports_512_nocombine", 7, 2, 6, 77, 3, [(21, 0.5)], 0.5, 20, combine=False,
                  idft_size=512, seed=5),
            Fresh("a3_120khz_zcz14_2ports_nocombine", 6, 3, 14, 9, 2, [(1, 0.3), (62, 0.6)], 0.1, 12, combine=False,
                  seed=6),
        ]
    return _fresh


def test_fresh_inputs_are_well_separated():
    """Precondition of the next test, on the model alone."""
    for c in fresh_cases():
        m = c.model()
        detected = {d[0] for d in m["detected"]}
        assert detected == {i for i, _ in c.tx if c.start <= i < c.start + c.nof}, c.name
        assert all(d[3] >= 1.2 for d in m["detected"]), c.name
        pot = m["peak_over_threshold"]
        assert all(not pot[i] > 0.9 for i in range(64) if i not in detected), c.name


def test_fresh_inputs_unaligned_offsets(detector, device):
    import torch

    cases = fresh_cases()
    sym, offsets = _pack([c.x for c in cases], [7, 13, 1, 33, 5, 63], device)
    assert all(o % 64 != 0 for o in offsets)
    raw = detector.detect_batch(sym, [_config(c) for c in cases], offsets)
    torch.cuda.synchronize()
    for res, c in zip(detector.results_to_host(raw), cases):
        _check_against_model(res, c.model(), c.start, c.start + c.nof, c.name)


def test_fresh_inputs_host_form(detector):
    for c in fresh_cases()[:2]:
        _check_against_model(detector.detect(c.x, _config(c)), c.model(), c.start, c.start + c.nof, c.name)


# ---- batch and stream behaviour ------------------------------------------------------------------------------------

def _raw(detector, sym, cfgs, offsets, stream=None):
    import torch

    out = detector.detect_batch(sym, cfgs, offsets, stream=stream)
    (stream or torch.cuda.current_stream()).synchronize()
    return out.cpu().numpy()


def test_same_occasion_33_times(detector, device):
    import torch

    fx = next(f for f in FIXTURES if f.name == "f0_zcz11_three_preambles")
    sym, offsets = _pack([fx.x] * 33, [3] * 33, device)
    raw = _raw(detector, sym, [_config(fx)] * 33, offsets)
    assert all(np.array_equal(raw[0], raw[i]) for i in range(1, 33))
    _check_fixture(detector.results_to_host(torch.from_numpy(raw))[32], fx)


def test_results_do_not_depend_on_batch_position(detector, device):
    picks = [FIXTURES[i] for i in (0, 6, 2, 11, 13)]
    sym, offsets = _pack([f.x for f in picks], [0] * len(picks), device)
    cfgs = [_config(f) for f in picks]
    a = _raw(detector, sym, cfgs, offsets)
    perm = [3, 0, 4, 2, 1]
    b = _raw(detector, sym, [cfgs[i] for i in perm], [offsets[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(b[j], a[i]), picks[i].name
    alone = _raw(detector, sym, [cfgs[2]], [offsets[2]])
    assert np.array_equal(alone[0], a[2])


def test_two_handles_on_two_streams(detector, device):
    import torch

    import srsran_project_amd as amd

    first, second = FIXTURES[:8], FIXTURES[8:]
    sym1, off1 = _pack([f.x for f in first], [0] * len(first), device)
    sym2, off2 = _pack([f.x for f in second], [0] * len(second), device)
    want1 = _raw(detector, sym1, [_config(f) for f in first], off1)
    want2 = _raw(detector, sym2, [_config(f) for f in second], off2)
    other = amd.PrachDetector(device.index or 0)
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        outs.append((detector.detect_batch(sym1, [_config(f) for f in first], off1, stream=s1),
                     other.detect_batch(sym2, [_config(f) for f in second], off2, stream=s2)))
    s1.synchronize()
    s2.synchronize()
    for o1, o2 in outs:
        assert np.array_equal(o1.cpu().numpy(), want1)
        assert np.array_equal(o2.cpu().numpy(), want2)
    other.close()


def test_second_call_with_other_root_uses_the_new_roots(device):
    """The root cache is keyed by (L_ra, u): a detector that has served root index 40 must correlate an occasion of
    root index 41 with the new roots (and 40 again afterwards)."""
    import srsran_project_amd as amd

    det = amd.PrachDetector(device.index or 0)
    a = Fresh("cache_root40", 0, 4, 9, 40, 2, [(20, 0.5)], 0.146, 5, seed=11)
    b = Fresh("cache_root41", 0, 4, 9, 41, 2, [(20, 0.5)], 0.146, 5, seed=12)
    for c in (a, b, a):
        res = det.detect(c.x, _config(c))
        _check_against_model(res, c.model(), 0, 64, c.name)
        assert [p.preamble_index for p in res.preambles] == [20]
    # b's input against a's roots holds no preamble of a's
    cross = det.detect(b.x, _config(a))
    m = pm.detect(pm.from_cbf16(b.x), 0, 4, 9, 40, 0, 64, 0.146, 5)
    assert [p.preamble_index for p in cross.preambles] == [d[0] for d in m["detected"]]
    det.close()


def test_invalid_configuration_launches_nothing(detector, device):
    import torch

    import srsran_project_amd as amd

    fx = FIXTURES[0]
    sym, offsets = _pack([fx.x, fx.x], [0, 0], device)
    results = torch.full((2, amd.prach.RESULT_BYTES), 0xA5, dtype=torch.uint8, device=device)
    for bad in (dict(zero_correlation_zone=16), dict(restricted_set=1), dict(start_preamble_index=1),
                dict(nof_rx_ports=0), dict(idft_size=768), dict(threshold=0.0), dict(win_margin=0),
                dict(win_margin=447)):
        with pytest.raises(ValueError):
            detector.detect_batch(sym, [_config(fx), _config(fx, **bad)], offsets, results=results)
        batch = amd.PrachBatch([_config(fx), _config(fx)], offsets)  # valid when prepared, then spoiled: the C call
        for k, v in bad.items():                                       # itself must refuse it
            setattr(batch.cfgs[1], k, v)
        with pytest.raises(ValueError):
            detector.detect_batch(sym, batch, results=results)
        with pytest.raises(ValueError):
            detector.detect(fx.x, _config(fx, **bad))
    torch.cuda.synchronize()
    assert bool((results == 0xA5).all())  # the valid first occasion was not launched either


def test_host_form_threads_on_one_handle_keep_their_own_input(detector):
    """Four threads in the host form of ONE detector, each with its own seeded occasion of the smallest fixture's
    configuration (tests/host_form_threads.py): every call returns its own thread's result bit for bit."""
    import struct

    from tests.host_form_threads import check_isolation

    fx = min(FIXTURES, key=lambda f: np.asarray(f.x).size)
    assert fx.name == "c0_15khz_zcz9_1port"
    cfg = _config(fx)
    occasions = [pm.make_occasion(np.random.default_rng(7000 + i), fx.format, fx.ra_scs, fx.zcz,
                                  fx.root_sequence_index, fx.ports, fx.tx, 1.0, fx.idft_size) for i in range(4)]

    def bits(r):
        pre = b"".join(struct.pack("2i3d", p.preamble_index, p.delay_samples, p.time_advance_s, p.detection_metric,
                                   p.preamble_power_db) for p in r.preambles)
        return (struct.pack("3d", r.rssi_db, r.time_resolution_s, r.time_advance_max_s) + pre +
                r.peak_over_threshold.tobytes() + r.delay_samples.tobytes())

    check_isolation(lambda x: detector.detect(x, cfg), occasions, bits)
