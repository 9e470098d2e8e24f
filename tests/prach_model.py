"""Float64 numpy restatement of the generic PRACH detector (TS 38.211 Section 6.3.3 preambles; the detection
statistic of prach_detector_generic_impl::detect), written from the algorithm's description: np.fft for the
transforms, root sequences from the direct Zadoff-Chu formula.  It shares no code with the library's kernels and
none with the reference; the tests hold the fixtures (tests/golden/prach_golden.npz, recorded from the reference)
and the GPU against it.

The logical-to-physical root order (Tables 6.3.3.1-3 / -4) is read from the fixture file, where it was recovered
from the reference's generated sequences -- the library's own table is checked against the same record.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prach_golden.npz")

FORMATS = ["0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3"]
SCS_HZ = [15000, 30000, 60000, 120000, 1250, 5000]  # ra_scs code -> Hz

# TS 38.211 Tables 6.3.3.1-1 / -2: (L_ra, nof_symbols = N_u / 2048 kappa 2^-mu, N_cp in units of kappa 2^-mu)
_LONG = {0: (1, 3168), 1: (2, 21024), 2: (4, 4688), 3: (4, 3168)}
_SHORT = {4: (2, 288), 5: (4, 576), 6: (6, 864), 7: (2, 216), 8: (12, 936), 9: (1, 1240), 10: (4, 2048),
          11: (2, 288), 12: (4, 576), 13: (6, 864)}
# TS 38.211 Tables 6.3.3.1-5 (1.25 kHz), -6 (5 kHz), -7 (15 kHz and above): N_cs, unrestricted sets
_NCS = {1250: [0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419],
        5000: [0, 13, 26, 33, 38, 41, 49, 55, 64, 76, 93, 119, 139, 209, 279, 419],
        0: [0, 2, 4, 6, 8, 10, 12, 13, 15, 17, 19, 23, 27, 34, 46, 69]}

T_C = 1.0 / (480000.0 * 4096.0)
KAPPA = 64
FLT_MIN = 1.17549435e-38

_roots = None


def physical_root(L_ra, logical):
    """u of logical root index i (wrapping at 838 / 138), from the fixture's record of both tables."""
    global _roots
    if _roots is None:
        z = np.load(GOLDEN)
        _roots = {839: z["roots_long"], 139: z["roots_short"]}
    t = _roots[L_ra]
    return int(t[logical % len(t)])


def quantize_time(seconds):
    """phy_time_unit::from_seconds(...).to_seconds(): the nearest whole number of T_c."""
    tc10 = int(seconds / T_C * 10.0)
    return float(tc10 // 10 + (tc10 % 10) // 5) * T_C


def geometry(fmt, ra_scs, zcz, idft_size=0):
    long_ = fmt < 4
    scs_hz = SCS_HZ[ra_scs]
    if long_:
        L, (nsym, ncp) = 839, _LONG[fmt]
        ncs = _NCS[scs_hz][zcz]
        cp_s = float(ncp * KAPPA) * T_C
    else:
        L, (nsym, ncp) = 139, _SHORT[fmt]
        ncs = _NCS[0][zcz]
        cp_s = float((ncp >> ra_scs) * KAPPA) * T_C
    N = idft_size or (1024 if long_ else 256)
    nof_shifts, nof_sequences = 1, 64
    if ncs:
        nof_shifts = min(64, L // ncs)
        nof_sequences = -(-64 // nof_shifts)
    cp_prach = int(math.floor(cp_s * L * scs_hz))
    win = cp_prach if ncs == 0 else min(ncs, cp_prach)
    md = cp_prach if ncs == 0 else min(max(ncs, 1) - 1, cp_prach)
    return dict(L_ra=L, N_cs=ncs, nof_shifts=nof_shifts, nof_sequences=nof_sequences, win_width=win * N // L,
                max_delay_samples=md * N // L, nof_symbols=nsym, idft_size=N, scs_hz=scs_hz)


def root_frequency_domain(L, u):
    """y_u[k] = sum_n x_u(n) exp(-j 2 pi n k / L), x_u(n) = exp(-j pi u n (n + 1) / L); |y_u| = sqrt(L)."""
    n = np.arange(L, dtype=np.int64)
    ph = (u * n * (n + 1)) % (2 * L)
    return np.fft.fft(np.exp(-1j * np.pi * ph / L))


def preamble_frequency_domain(L, u, cyclic_shift):
    """y_{u,v}: x_{u,v}(n) = x_u((n + C_v) mod L)."""
    n = (np.arange(L, dtype=np.int64) + cyclic_shift) % L
    ph = (u * n * (n + 1)) % (2 * L)
    return np.fft.fft(np.exp(-1j * np.pi * ph / L))


def make_occasion(rng, fmt, ra_scs, zcz, root_sequence_index, nof_ports, preambles, noise_sigma, idft_size=0,
                  amplitude=1.0):
    """Seeded test input: `preambles` = [(preamble index, delay in IDFT samples)], one random phase per port, complex
    noise, rounded to bf16.  Returns uint16 [ports, symbols, L_ra, 2]."""
    g = geometry(fmt, ra_scs, zcz, idft_size)
    L, N = g["L_ra"], g["idft_size"]
    x = np.zeros((nof_ports, g["nof_symbols"], L), np.complex128)
    k = np.arange(L) - L // 2
    for idx, delay in preambles:
        if g["N_cs"]:
            per_root = L // g["N_cs"]
            u = physical_root(L, root_sequence_index + idx // per_root)
            shift = (idx % per_root) * g["N_cs"]
        else:
            u, shift = physical_root(L, root_sequence_index + idx), 0
        y = preamble_frequency_domain(L, u, shift) / math.sqrt(L) * amplitude * np.exp(-2j * np.pi * k * delay / N)
        x += y[None, None, :] * np.exp(2j * np.pi * rng.random(nof_ports))[:, None, None]
    x += (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * (noise_sigma / math.sqrt(2.0))
    return to_cbf16(x)


def to_cbf16(x):
    """complex -> uint16 [..., 2] bf16 bit patterns, round half to even."""
    f = np.stack([x.real, x.imag], axis=-1).astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return b.astype(np.uint16)


def from_cbf16(x):
    """uint16 [..., 2] bf16 bit patterns -> complex128."""
    f = (np.asarray(x, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f[..., 0] + 1j * f[..., 1]


def detect(x, fmt, ra_scs, zcz, root_sequence_index, start, nof, threshold, win_margin, combine_symbols=True,
           idft_size=0):
    """x: complex [ports, symbols, L_ra].  Returns a dict: rssi_db, time_resolution_s, time_advance_max_s,
    detected = [(preamble_index, delay_samples, time_advance_s, detection_metric, preamble_power_db)],
    peak_over_threshold [64] (NaN outside the range), delay_samples [64] (-1 outside the range)."""
    g = geometry(fmt, ra_scs, zcz, idft_size)
    L, N, ncs = g["L_ra"], g["idft_size"], g["N_cs"]
    W, nsh = g["win_width"], g["nof_shifts"]
    x = np.asarray(x, np.complex128)
    ports, nsym = x.shape[0], x.shape[1]
    assert nsym == g["nof_symbols"] and x.shape[2] == L
    fs = float(N * g["scs_hz"])
    rssi = float(np.mean(np.abs(x) ** 2))
    with np.errstate(divide="ignore"):
        out = dict(rssi_db=10.0 * math.log10(rssi) if rssi > 0 else -math.inf,
                   time_resolution_s=quantize_time(1.0 / fs),
                   time_advance_max_s=quantize_time(g["max_delay_samples"] * 0.8 / fs),
                   detected=[], peak_over_threshold=np.full(64, np.nan), delay_samples=np.full(64, -1, np.int64))
    if not (rssi >= FLT_MIN and math.isfinite(rssi)):
        return out
    sym = x.sum(axis=1, keepdims=True) if combine_symbols else x
    for i_seq in range(g["nof_sequences"]):
        lo, hi = i_seq * nsh, (i_seq + 1) * nsh
        if not (lo < start + nof and start < hi):
            continue
        yc = np.conj(root_frequency_domain(L, physical_root(L, root_sequence_index + i_seq)))
        num = np.zeros((nsh, W))
        den = np.zeros((nsh, W))
        for p in range(ports):
            for s in range(sym.shape[1]):
                prod = sym[p, s] * yc
                v = np.zeros(N, np.complex128)
                v[:L // 2 + 1] = prod[L - (L // 2 + 1):]
                v[N - L // 2:] = prod[:L // 2]
                ms = np.abs(np.fft.ifft(v) * N) ** 2 / float(N * L)
                for w in range(nsh):
                    ws = (N - (ncs * w * N) // L) % N
                    idx = (ws - win_margin + np.arange(2 * win_margin + W)) % N
                    ref = ms[idx].sum()
                    win = ms[ws:ws + W] * (float(N) / float(L))
                    diff = ref - win
                    diff = np.where(np.isfinite(diff) & (np.abs(diff) >= FLT_MIN), diff, 1e-9)
                    num[w] += win
                    den[w] += diff
        for w in range(nsh):
            idx = lo + w
            if not (start <= idx < start + nof):
                continue
            metric = num[w] / np.abs(den[w])
            delay = int(np.argmax(metric))
            peak = float(metric[delay])
            out["peak_over_threshold"][idx] = peak / threshold
            out["delay_samples"][idx] = delay
            if peak > threshold and delay < g["max_delay_samples"] * 0.8:
                norm = ports * L * nsym * (nsym if combine_symbols else 1)
                out["detected"].append((idx, delay, quantize_time(delay / fs), peak / threshold,
                                        10.0 * math.log10(num[w, delay] / norm)))
    return out


class Fixture:
    """One case of tests/golden/prach_golden.npz."""

    def __init__(self, z, i, name):
        k = "c%02d_" % i
        self.name = name
        (self.format, self.ra_scs, self.root_sequence_index, self.zcz, self.start, self.nof, self.ports, combine,
         self.idft_size, accepted) = (int(v) for v in z[k + "cfg"])
        self.combine = bool(combine)
        self.validator_accepts = bool(accepted)
        self.geo = dict(zip(["L_ra", "N_cs", "nof_shifts", "nof_sequences", "win_width", "max_delay_samples",
                             "nof_symbols", "win_margin"], (int(v) for v in z[k + "geo"])))
        self.win_margin = self.geo["win_margin"]
        self.threshold = float(z[k + "thr"][0])
        self.x = z[k + "x"]
        self.tx = [tuple(int(v) for v in r) for r in z[k + "tx"]]
        self.rssi_db, self.time_resolution_s, self.time_advance_max_s = (float(v) for v in z[k + "res"])
        self.det = z[k + "det"]

    def model(self):
        return detect(from_cbf16(self.x), self.format, self.ra_scs, self.zcz, self.root_sequence_index, self.start,
                      self.nof, self.threshold, self.win_margin, self.combine, self.idft_size)


_fixtures = None


def fixtures():
    """The fixture cases, loaded once."""
    global _fixtures
    if _fixtures is None:
        z = np.load(GOLDEN)
        names = bytes(z["names"]).decode().split("\n")
        _fixtures = [Fixture(z, i, n) for i, n in enumerate(names)]
    return _fixtures


_model_results = {}


def model_of(fx):
    """The float64 model's result for a fixture, computed once and shared (read-only) among the tests."""
    if fx.name not in _model_results:
        _model_results[fx.name] = fx.model()
    return _model_results[fx.name]


def reference_deviation():
    """Largest deviation of the recorded float32 reference from the float64 model over all fixtures:
    (relative on detection_metric, absolute dB on preamble_power_db, absolute dB on rssi_db)."""
    dm = dp = dr = 0.0
    for fx in fixtures():
        m = model_of(fx)
        if math.isfinite(fx.rssi_db):
            dr = max(dr, abs(fx.rssi_db - m["rssi_db"]))
        by_idx = {d[0]: d for d in m["detected"]}
        for idx, _, metric, power in fx.det:
            d = by_idx.get(int(idx))
            if d is not None:
                dm = max(dm, abs(metric - d[3]) / d[3])
                dp = max(dp, abs(power - d[4]))
    return dm, dp, dr
