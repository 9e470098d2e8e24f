"""Float64 numpy restatement of the SRS channel estimator (TS 38.211 Section 6.4.1.4 sequences and mapping; the
estimator of srs_estimator_generic_impl::estimate with the DFT-based time-alignment estimator), written from the
algorithm's description: np.fft for the transforms, base sequences from the Zadoff-Chu formula of Section 5.2.2.  It
shares no code with the library's kernels and none with the reference; the tests hold the fixtures
(tests/golden/srs_golden.npz, recorded from the reference by tools/srs_golden_gen.cpp) and the GPU against it.

Two things are part of the algorithm and therefore restated as they are, not idealised:
  * the phase compensation reads a 1024-entry table exp(j 2 pi k / 1024) at the index
    round(1024 (n phase_shift_subcarrier + phase_shift_offset) / 2 pi), the index computed in float32;
  * the peak rule: the first maximum of the delayed taps [0, m) and of the advanced taps [N - m, N), the delayed one
    on a tie, then a 5-tap (3-tap for m <= 2) quadratic refinement with the weights written as six-digit decimals.

The bandwidth table (TS 38.211 Table 6.4.1.4.3-1) is read from the fixture file, where the generator recorded the
reference's; the phase tables of the sequences of length 6 .. 24 (Tables 5.2.2.2-1 .. -4) from the library's
facts-only include file.
"""
import math
import os
import re
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "srs_golden.npz")
PHI_TABLES = os.path.join(HERE, "..", "srsran_project_amd", "csrc", "low_papr_tables.inc")

T_C = 1.0 / (480000.0 * 4096.0)
NSYMB = 14
CEXP_SIZE = 1024
CFG_FIELDS = ("nof_antenna_ports", "nof_symbols", "start_symbol", "configuration_index", "sequence_id",
              "bandwidth_index", "comb_size", "comb_offset", "cyclic_shift", "freq_position", "freq_shift",
              "freq_hopping", "numerology")

_npz = None
_phi = None


def golden():
    global _npz
    if _npz is None:
        _npz = np.load(GOLDEN)
    return _npz


def bandwidth(c_srs, b_srs):
    """(m_SRS, N) as the fixture file records them."""
    t = golden()["bandwidth"]
    return int(t[c_srs, b_srs, 0]), int(t[c_srs, b_srs, 1])


class Config:
    """The fields of srs_estimator_configuration the estimator reads."""

    def __init__(self, rx_ports=(0,), hopping=0, **kw):
        for f in CFG_FIELDS:
            setattr(self, f, int(kw.pop(f, 0)))
        assert not kw, kw
        self.rx_ports = [int(p) for p in rx_ports]
        self.hopping = int(hopping)

    def library(self, **over):
        """The same configuration for the Python layer of the library."""
        import srsran_project_amd as amd

        kw = {f: getattr(self, f) for f in CFG_FIELDS}
        kw.update(rx_ports=list(self.rx_ports), hopping=self.hopping)
        kw.update(over)
        return amd.SrsConfiguration(**kw)


def information(cfg, antenna_port):
    """TS 38.211 Section 6.4.1.4.2 / 6.4.1.4.3 without hopping: (M, u, v, n_cs, n_cs_max, k_0, K_TC)."""
    comb = cfg.comb_size
    m_srs, _ = bandwidth(cfg.configuration_index, cfg.bandwidth_index)
    M = m_srs * 12 // comb
    n_cs_max = 12 if comb == 4 else 8
    n_cs = (cfg.cyclic_shift + n_cs_max * antenna_port // cfg.nof_antenna_ports) % n_cs_max
    k_tc = cfg.comb_offset
    if cfg.nof_antenna_ports == 4 and antenna_port in (1, 3) and n_cs_max // 2 <= cfg.cyclic_shift < n_cs_max:
        k_tc = (k_tc + comb // 2) % comb
    k0 = cfg.freq_shift * 12 + k_tc
    for b in range(cfg.bandwidth_index + 1):
        m_b, N_b = bandwidth(cfg.configuration_index, b)
        k0 += comb * (m_b * 12 // comb) * ((4 * cfg.freq_position // m_b) % N_b)
    return M, cfg.sequence_id % 30, 0, n_cs, n_cs_max, k0, comb


def idft_size(M):
    need, n = M * 4096 // 3300, 128
    while n < need:
        n *= 2
    return n


def _phi_table(M):
    global _phi
    if _phi is None:
        text = open(PHI_TABLES).read()
        _phi = {}
        for m in re.finditer(r"SRS_LOW_PAPR_PHI_(\d+)\[30\]\[\d+\]\s*=\s*\{(.*?)\};", text, re.S):
            rows = re.findall(r"\{([^{}]*)\}", m.group(2))
            _phi[int(m.group(1))] = np.array([[int(v) for v in r.split(",")] for r in rows])
    return _phi[M]


def _largest_prime_below(n):
    p = n - 1
    while any(p % d == 0 for d in range(2, int(math.isqrt(p)) + 1)):
        p -= 1
    return p


def base_sequence(M, u, v=0):
    """r_{u,v}(n) of TS 38.211 Section 5.2.2, float64."""
    n = np.arange(M, dtype=np.int64)
    if M <= 24:
        return np.exp(1j * np.pi * _phi_table(M)[u] / 4.0)
    if M == 30:
        return np.exp(-1j * np.pi * (((u + 1) * (n + 1) * (n + 2)) % 62) / 31.0)
    nzc = _largest_prime_below(M)
    q_bar = Fraction(nzc * (u + 1), 31)
    q = math.floor(q_bar + Fraction(1, 2)) + v * (-1) ** math.floor(2 * q_bar)
    m = n % nzc
    return np.exp(-1j * np.pi * ((q * m * (m + 1)) % (2 * nzc)) / nzc)


def pilots(cfg, antenna_port):
    """The sequence of one antenna port, cyclic shift alpha = 2 pi n_cs / n_cs_max applied."""
    M, u, v, n_cs, n_cs_max, _, _ = information(cfg, antenna_port)
    n = np.arange(M)
    return base_sequence(M, u, v) * np.exp(2j * np.pi * ((n * n_cs) % n_cs_max) / n_cs_max)


def from_cbf16(x):
    """uint16 [..., 2] bf16 bit patterns -> complex128."""
    f = (np.asarray(x, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f[..., 0] + 1j * f[..., 1]


def to_cbf16(x):
    """complex array -> uint16 [..., 2] bf16 bit patterns (real, imaginary), round half to even."""
    f = np.stack([np.real(x), np.imag(x)], axis=-1).astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def ta_range(cfg):
    """(N, sampling rate, max_ta_samples) of the time-alignment stage."""
    M, _, _, _, n_cs_max, _, comb = information(cfg, 0)
    N = idft_size(M)
    scs = 15000 << cfg.numerology
    rate = float(N * scs * comb)
    half_cp = ((144 * 64) >> (cfg.numerology + 1)) * T_C
    max_ta = 1.0 / float(n_cs_max * scs * comb)
    return N, rate, min(int(math.floor(half_cp * rate)), int(math.floor(max_ta * rate)))


def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def _phase_table_entries(M, phase_sub, phase_off):
    """compensate_phase_shift: float32 index arithmetic, exact table entries."""
    n = np.arange(M, dtype=np.float32)
    arg = (n * np.float32(phase_sub)).astype(np.float32) + np.float32(phase_off)
    x = (np.float32(CEXP_SIZE) * arg.astype(np.float32)).astype(np.float32) / np.float32(2.0 * np.float32(np.pi))
    idx = _round_half_away(x.astype(np.float32)).astype(np.int64) % CEXP_SIZE
    return np.exp(2j * np.pi * idx / CEXP_SIZE)


def _peak(corr, m):
    """(integer tap, fractional tap) of one correlation."""
    N = len(corr)
    i_d, i_a = int(np.argmax(corr[:m])), int(np.argmax(corr[N - m:]))
    idx = i_d if corr[i_d] >= corr[N - m + i_a] else -(m - i_a)
    taps = 5 if m > 2 else 3
    pk = np.array([corr[(idx + i + N - taps // 2) % N] for i in range(taps)])
    if taps == 5:
        num = np.dot([-0.4, -0.2, 0.0, 0.2, 0.4], pk)
        den = np.dot([0.571429, -0.285714, -0.571429, -0.285714, 0.571429], pk)
        corr_f = 1.0
    else:
        num = np.dot([-0.5, 0.0, 0.5], pk)
        den = np.dot([0.5, -1.0, 0.5], pk)
        corr_f = 0.5
    with np.errstate(all="ignore"):
        f = -corr_f * num / den
    if not np.isfinite(f) or abs(f) > 1.0:
        f = 0.0
    return idx, float(f)


def estimate(rows, cfg):
    """rows: complex [nof_rx_ports, nof_symbols, nof_subc], the grid rows of the SRS symbols by rx port index.
    Returns a dict with the fields of srs_estimator_result and the intermediate time-alignment data."""
    rows = np.asarray(rows, np.complex128)
    nrx, nsym, _ = rows.shape
    nap = cfg.nof_antenna_ports
    assert nsym == cfg.nof_symbols and nrx == len(cfg.rx_ports)
    infos = [information(cfg, p) for p in range(nap)]
    M, comb = infos[0][0], infos[0][6]
    seqs = [pilots(cfg, p) for p in range(nap)]
    N, rate, m = ta_range(cfg)
    scs = 15000 << cfg.numerology
    interleaved = nap == 4 and infos[0][3] >= infos[0][4] // 2

    def received(p):  # [nrx, nsym, M]
        k0 = infos[p][5]
        return rows[:, :, k0:k0 + comb * M:comb]

    lse = np.empty((nrx, nap, M), np.complex128)
    ta_ports, idx_ports, corrs = [], [], []
    for p in range(nap):
        lse[:, p, :] = received(p).sum(axis=1) * np.conj(seqs[p]) / nsym
        corr = np.zeros(N)
        for r in range(nrx):
            corr += np.abs(np.fft.ifft(lse[r, p], N) * N) ** 2
        idx, frac = _peak(corr, m)
        ta_ports.append((idx + frac) / rate)
        idx_ports.append(idx)
        corrs.append(corr)
    ta = sum(ta_ports) / nap

    phase_sub = np.float32(float(np.float32(2.0 * np.float32(np.pi))) * ta * (scs // 1000) * 1000 * comb)
    coef = np.zeros((nrx, nap), np.complex128)
    noise, epre = 0.0, 0.0
    sets = [0, 1] if interleaved else [0]
    for r in range(nrx):
        residual = {}
        for s in sets:
            rx = received(s)[r]
            epre += float(np.sum(np.mean(np.abs(rx) ** 2, axis=1)))
            off = np.float32(phase_sub * np.float32(infos[s][5])) / np.float32(comb)
            residual[s] = rx.sum(axis=0) * _phase_table_entries(M, phase_sub, off)
        for p in range(nap):
            off = np.float32(phase_sub * np.float32(infos[p][5])) / np.float32(comb)
            coef[r, p] = np.mean(lse[r, p] * _phase_table_entries(M, phase_sub, off))
            residual[p % 2 if interleaved else 0] -= nsym * coef[r, p] * seqs[p]
        noise += sum(float(np.sum(np.abs(v) ** 2)) for v in residual.values())
    rsrp = float(np.sum(np.abs(coef) ** 2))
    nof_estimates, correction = (2, 2) if interleaved else (nap, 1)
    noise /= (nsym * M - nof_estimates) * correction * nrx
    with np.errstate(all="ignore"):
        noise_std = max(math.sqrt(noise), 0.01 * math.sqrt(rsrp))
        matrix = coef * (np.float64(1.0) / np.float64(noise_std))
        epre /= nsym * correction * nrx
        rsrp /= nap * nrx
        epre_db = float(10.0 * np.log10(np.float64(epre)))
        rsrp_db = float(10.0 * np.log10(np.float64(rsrp)))
    return dict(matrix=matrix, epre_db=epre_db, rsrp_db=rsrp_db, noise_variance=noise, time_alignment_s=ta,
                ta_resolution_s=1.0 / rate, ta_max_s=m / rate, ta_ports=ta_ports, idx_ports=idx_ports, corr=corrs,
                max_ta_samples=m, idft_size=N, sampling_rate=rate)


def peak_margin(model):
    """Smallest ratio, over the antenna ports, of the integer correlation peak to the largest sample more than two
    taps away from it inside the two search ranges."""
    m, worst = model["max_ta_samples"], math.inf
    for corr, idx in zip(model["corr"], model["idx_ports"]):
        N = len(corr)
        taps = np.concatenate([np.arange(m), np.arange(N - m, N)])
        signed = np.where(taps < m, taps, taps - N)
        far = np.abs(signed - idx) > 2
        if corr[idx % N] == 0.0 or not far.any():
            continue
        worst = min(worst, corr[idx % N] / max(corr[taps[far]].max(), 1e-300))
    return worst


# ---- fixtures --------------------------------------------------------------------------------------------------------

class Fixture:
    def __init__(self, z, i, name):
        k = "c%02d_" % i
        cfg = [int(v) for v in z[k + "cfg"]]
        self.name = name
        nrx = cfg[13]
        self.cfg = Config(rx_ports=cfg[14:14 + nrx], **dict(zip(CFG_FIELDS, cfg[:13])))
        self.nof_subc = cfg[18]
        self.x = z[k + "x"]  # uint16 [nof_rx, nof_symbols, nof_subc, 2]
        self.h = z[k + "h"][..., 0] + 1j * z[k + "h"][..., 1]
        self.delay_s, self.noise_sigma = (float(v) for v in z[k + "chan"])
        self.matrix = (z[k + "mat"][..., 0] + 1j * z[k + "mat"][..., 1]).astype(np.complex64)
        self.epre_db, self.rsrp_db, self.noise_variance = (np.float32(v) for v in z[k + "pow"])
        self.time_alignment_s, self.ta_resolution_s, self.ta_min_s, self.ta_max_s = (float(v) for v in z[k + "ta"])
        self.all_zero = not self.x.any()
        self._model = None

    def model(self):
        if self._model is None:
            self._model = estimate(from_cbf16(self.x), self.cfg)
        return self._model


_fixtures = None


def fixtures():
    global _fixtures
    if _fixtures is None:
        z = golden()
        names = bytes(z["names"]).decode().split("\n")
        _fixtures = [Fixture(z, i, n) for i, n in enumerate(names)]
    return _fixtures


def used_mask(cfg, nof_subc):
    """bool [nof_subc]: the subcarriers any antenna port of the PDU occupies."""
    mask = np.zeros(nof_subc, bool)
    for p in range(cfg.nof_antenna_ports):
        M, _, _, _, _, k0, comb = information(cfg, p)
        mask[k0:k0 + comb * M:comb] = True
    return mask


def build_grid(x, cfg, nof_grid_ports, seed, nof_subc=None, keep_rows=False):
    """The 14-symbol grid around the recorded (or generated) rows x (uint16 [nof_rx, nof_symbols, nof_subc, 2]):
    seeded non-zero garbage in every other symbol, in the ports not listed, beyond the rows' end when the grid is
    wider (nof_subc) and -- unless keep_rows -- on the subcarriers of the SRS symbols the PDU does not use, so that a
    wrong stride, offset or port shows."""
    rng = np.random.default_rng(seed)
    nrx, nsym, width, _ = x.shape
    nof_subc = nof_subc or width
    grid = to_cbf16((rng.standard_normal((nof_grid_ports, NSYMB, nof_subc)) +
                     1j * rng.standard_normal((nof_grid_ports, NSYMB, nof_subc))) * 3.0 + (2.0 - 1.0j))
    keep = np.ones(width, bool) if keep_rows else used_mask(cfg, width)
    for r in range(nrx):
        for s in range(nsym):
            grid[cfg.rx_ports[r], cfg.start_symbol + s, :width][keep] = np.asarray(x[r, s], np.uint16)[keep]
    return grid


def make_complex_rows(rng, cfg, nof_subc, delay_fraction, sigma, amplitude=1.0):
    """A seeded reception for `cfg`: one complex coefficient per (rx, tx), a common delay (a fraction of the
    measurable range), complex Gaussian noise on every subcarrier; complex [nof_rx, nof_symbols, nof_subc]."""
    nrx, nap, nsym = len(cfg.rx_ports), cfg.nof_antenna_ports, cfg.nof_symbols
    _, rate, m = ta_range(cfg)
    delay = delay_fraction * m / rate
    scs = 15000 << cfg.numerology
    h = amplitude * (0.5 + rng.random((nrx, nap))) * np.exp(2j * np.pi * rng.random((nrx, nap)))
    clean = np.zeros((nrx, nof_subc), np.complex128)
    for p in range(nap):
        M, _, _, _, _, k0, comb = information(cfg, p)
        k = k0 + comb * np.arange(M)
        clean[:, k] += h[:, p, None] * pilots(cfg, p) * np.exp(-2j * np.pi * k * scs * delay)
    noise = rng.standard_normal((nrx, nsym, nof_subc)) + 1j * rng.standard_normal((nrx, nsym, nof_subc))
    return clean[:, None, :] + noise * (sigma / math.sqrt(2.0))


def make_rows(rng, cfg, nof_subc, delay_fraction, sigma, amplitude=1.0):
    """make_complex_rows rounded to cbf16: uint16 [nof_rx, nof_symbols, nof_subc, 2]."""
    return to_cbf16(make_complex_rows(rng, cfg, nof_subc, delay_fraction, sigma, amplitude))


def reference_deviation():
    """Largest deviation of the recorded float32 reference from this model over the fixtures (the all-zero one
    aside): (matrix coefficients relative to the Frobenius norm of the case's matrix, noise_variance relative,
    epre_dB in dB, rsrp_dB in dB, time alignment in IDFT samples -- the integer taps agree, so this is the fractional
    part)."""
    dev = np.zeros(5)
    for fx in fixtures():
        if fx.all_zero:
            continue
        m = fx.model()
        dev[0] = max(dev[0], np.abs(fx.matrix - m["matrix"]).max() / np.linalg.norm(m["matrix"]))
        dev[1] = max(dev[1], abs(float(fx.noise_variance) - m["noise_variance"]) / m["noise_variance"])
        dev[2] = max(dev[2], abs(float(fx.epre_db) - m["epre_db"]))
        dev[3] = max(dev[3], abs(float(fx.rsrp_db) - m["rsrp_db"]))
        dev[4] = max(dev[4], abs(fx.time_alignment_s - m["time_alignment_s"]) / m["ta_resolution_s"])
    return tuple(float(v) for v in dev)
