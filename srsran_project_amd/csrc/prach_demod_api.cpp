// prach_demod_api.cpp -- C-ABI of the MI355X PRACH OFDM demodulator (include/srsran_amd/prach_demodulator.h): the
// timing and frequency geometry of ofdm_prach_demodulator_impl::demodulate (ofdm_prach_demodulator_impl.cpp:78-195)
// and get_prach_window_duration (prach_preamble_information.cpp:117-169), the DFT plans and the launch sequence of
// prach_demod.hip.
#include "srsran_amd/prach_demodulator.h"
#include "srsran_amd/ldpc.h"

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "device_buffer.h"
#include "prach_demod_args.h"
#include "staged_call.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace srs_amd;

namespace {

// Times are whole numbers of kappa = 64 T_c = 1 / 30.72 MHz (every quantity the reference handles here is one).
constexpr uint64_t KAPPA_RATE_HZ = 30720000;
constexpr uint64_t HALF_MS       = 15360;
constexpr uint64_t SIXTEEN       = 16;
constexpr uint32_t MAX_D         = 192;
constexpr uint32_t MAX_PORTS     = 255;

// Preamble formats in the order of srs_amd_prach_format: TS 38.211 Tables 6.3.3.1-1 and 6.3.3.1-2.  cp / cp_last in
// kappa 2^-mu (mu = 0 for the long formats); cp_last is the prefix of the last time-domain occasion (the B prefix of
// the A/B formats); duration: OFDM symbols a time-domain occasion takes (get_preamble_duration).
struct format_row {
  uint16_t L_ra, nof_symbols, cp, cp_last, duration;
};
constexpr format_row FORMATS[14] = {
    {839, 1, 3168, 3168, 0},   // 0
    {839, 2, 21024, 21024, 0}, // 1
    {839, 4, 4688, 4688, 0},   // 2
    {839, 4, 3168, 3168, 0},   // 3
    {139, 2, 288, 288, 2},     // A1
    {139, 4, 576, 576, 4},     // A2
    {139, 6, 864, 864, 6},     // A3
    {139, 2, 216, 216, 2},     // B1
    {139, 12, 936, 936, 12},   // B4
    {139, 1, 1240, 1240, 2},   // C0
    {139, 4, 2048, 2048, 6},   // C2
    {139, 2, 288, 216, 2},     // A1/B1
    {139, 4, 576, 360, 4},     // A2/B2
    {139, 6, 864, 504, 6},     // A3/B3
};

// prach_frequency_mapping_get (TS 38.211 Table 6.3.3.2-1): N_RB^RA and k_bar by PUSCH numerology; 0: reserved.
struct mapping_row {
  uint16_t nof_rb_ra, k_bar;
};
constexpr mapping_row MAP_1_25[4] = {{6, 7}, {3, 1}, {2, 133}, {0, 0}};
constexpr mapping_row MAP_5[4]    = {{24, 12}, {12, 10}, {6, 7}, {0, 0}};
constexpr mapping_row MAP_SHORT   = {12, 2}; // RA spacing = PUSCH spacing, 15 to 120 kHz

bool srate_supported(uint32_t srate)
{
  if (srate % 15000u != 0) {
    return false;
  }
  uint32_t q = srate / 15000u;
  if (q < 128 || q > 16384) {
    return false;
  }
  while ((q & 1u) == 0) {
    q >>= 1;
  }
  return q == 1 || q == 3;
}

// dft_size -> (M, D); false when there is neither a plan nor a split
bool dft_plan(uint32_t N, uint32_t& M, uint32_t& D)
{
  if (prach_demod_planned(N)) {
    M = N;
    D = 1;
    return true;
  }
  for (uint32_t m : {1024u, 512u, 256u}) {
    if (N % m == 0 && N / m <= MAX_D && N / m >= 2) {
      M = m;
      D = N / m;
      return true;
    }
  }
  return false;
}

// adjacent residues per workgroup: the largest divisor of D that fits the workgroup
uint32_t residues_per_group(uint32_t D)
{
  for (uint32_t a = PRACH_DEMOD_MAX_A; a > 1; --a) {
    if (D % a == 0) {
      return a;
    }
  }
  return 1;
}

// phy_time_unit::to_samples: false when the time is not a whole number of samples
bool to_samples(uint64_t kappa, uint32_t srate, uint64_t& samples)
{
  const uint64_t p = kappa * srate;
  samples          = p / KAPPA_RATE_HZ;
  return p % KAPPA_RATE_HZ == 0;
}

struct derived {
  srs_amd_prach_demod_geometry g;
  uint32_t                     k_step, half;
};

int derive(uint32_t srate, const srs_amd_prach_demod_config& c, derived& d)
{
  if (c.format > SRS_AMD_PRACH_FORMAT_A3_B3) {
    return fail(SRS_AMD_EINVAL, "Invalid PRACH format (i.e., %u).", c.format);
  }
  if (c.numerology > 3 || c.subframe_slot_index >= (1u << c.numerology) || c.start_symbol >= 14) {
    return fail(SRS_AMD_EINVAL, "Invalid slot (numerology %u, slot %u in the subframe) or start symbol (i.e., %u).",
                c.numerology, c.subframe_slot_index, c.start_symbol);
  }
  const format_row& f       = FORMATS[c.format];
  const bool        is_long = c.format <= SRS_AMD_PRACH_FORMAT_3;
  if (c.nof_td_occasions == 0) {
    return fail(SRS_AMD_EINVAL, "The number of time-domain occasions must be greater than 0.");
  }
  if (is_long && c.nof_td_occasions != 1) {
    return fail(SRS_AMD_EINVAL, "Long preambles only support one occasion.");
  }
  if (c.nof_td_occasions > SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS) {
    return fail(SRS_AMD_EINVAL, "The number of time-domain occasions (i.e., %u) exceeds the maximum (i.e., %u).",
                c.nof_td_occasions, SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS);
  }
  if (c.nof_fd_occasions == 0 || c.nof_fd_occasions > SRS_AMD_PRACH_DEMOD_MAX_FD_OCCASIONS) {
    return fail(SRS_AMD_EINVAL, "The number of frequency-domain occasions (i.e., %u) must be 1 to %u.",
                c.nof_fd_occasions, SRS_AMD_PRACH_DEMOD_MAX_FD_OCCASIONS);
  }
  if (c.nof_ports == 0 || c.nof_ports > MAX_PORTS) {
    return fail(SRS_AMD_EINVAL, "The number of ports (i.e., %u) must be 1 to %u.", c.nof_ports, MAX_PORTS);
  }
  if (!srate_supported(srate)) {
    return fail(SRS_AMD_EINVAL, "Unsupported sampling rate %u Hz.", srate);
  }
  srs_amd_prach_demod_geometry& g = d.g;
  std::memset(&g, 0, sizeof(g));
  const uint32_t mu       = c.numerology;
  const uint32_t pusch_hz = 15000u << mu;
  uint32_t       ra_hz;
  mapping_row    map;
  if (c.format <= SRS_AMD_PRACH_FORMAT_2) {
    g.ra_scs = SRS_AMD_PRACH_SCS_1_25KHZ;
    ra_hz    = 1250;
    map      = MAP_1_25[mu];
  } else if (c.format == SRS_AMD_PRACH_FORMAT_3) {
    g.ra_scs = SRS_AMD_PRACH_SCS_5KHZ;
    ra_hz    = 5000;
    map      = MAP_5[mu];
  } else {
    g.ra_scs = mu; // to_ra_subcarrier_spacing(pusch_scs)
    ra_hz    = pusch_hz;
    map      = MAP_SHORT;
  }
  if (map.nof_rb_ra == 0) {
    return fail(SRS_AMD_EINVAL,
                "The PRACH and PUSCH subcarrier spacing combination resulted in a reserved configuration.");
  }
  if (srate % ra_hz != 0 || !dft_plan(srate / ra_hz, g.sub_dft_size, g.nof_sub_dfts)) {
    return fail(SRS_AMD_EINVAL, "No DFT of %u Hz / %u Hz points.", srate, ra_hz);
  }
  g.L_ra        = f.L_ra;
  g.dft_size    = srate / ra_hz;
  g.nof_symbols = f.nof_symbols;

  // frequency domain (ofdm_prach_demodulator_impl.cpp:165-194)
  const uint64_t K    = pusch_hz / ra_hz;
  const uint64_t grid = static_cast<uint64_t>(c.nof_prb_ul_grid) * K * 12;
  if (g.dft_size <= grid) {
    return fail(SRS_AMD_EINVAL, "DFT size %u is not sufficient for K=%u, N_RB=%u.", g.dft_size,
                static_cast<unsigned>(K), c.nof_prb_ul_grid);
  }
  d.k_step = static_cast<uint32_t>(K * 12 * map.nof_rb_ra);
  d.half   = static_cast<uint32_t>(grid / 2);
  for (uint32_t i = 0; i != c.nof_fd_occasions; ++i) {
    const uint64_t k_start = K * 12 * (static_cast<uint64_t>(c.rb_offset) + map.nof_rb_ra * i) + map.k_bar;
    if (k_start + g.L_ra >= grid) {
      return fail(SRS_AMD_EINVAL, "Start subcarrier %llu plus sequence length %u exceeds PRACH grid size %llu.",
                  static_cast<unsigned long long>(k_start), g.L_ra, static_cast<unsigned long long>(grid));
    }
    g.k_start[i] = static_cast<uint32_t>(k_start);
  }

  // time domain (ofdm_prach_demodulator_impl.cpp:78-135)
  const uint64_t symbol   = 2192u >> mu; // PUSCH symbol, kappa
  const uint64_t t_slot   = symbol * c.subframe_slot_index * 14;
  const uint64_t ra_sym   = g.ra_scs == SRS_AMD_PRACH_SCS_1_25KHZ ? 24576u : g.ra_scs == SRS_AMD_PRACH_SCS_5KHZ ? 6144u
                                                                                                               : 2048u >> mu;
  const uint64_t sym_len  = ra_sym * f.nof_symbols;
  const bool     low_scs  = is_long || mu <= 1; // 1.25, 5, 15 and 30 kHz
  for (uint32_t i = 0; i != c.nof_td_occasions; ++i) {
    const bool last    = i + 1 == c.nof_td_occasions;
    uint64_t   cp      = is_long ? f.cp : static_cast<uint64_t>(last ? f.cp_last : f.cp) >> mu;
    uint64_t   t_occ   = symbol * (c.start_symbol + f.duration * i);
    const uint64_t t_ra_start = t_occ + t_slot;
    if (low_scs) {
      if (t_occ > 0) {
        t_occ += SIXTEEN;
      }
      if (t_occ > HALF_MS) {
        t_occ += SIXTEEN;
      }
    }
    const uint64_t t_ra_end = t_ra_start + cp + sym_len;
    if (!is_long) {
      if (t_ra_start == 0) {
        cp += SIXTEEN;
      }
      if (t_ra_start <= HALF_MS && t_ra_end >= HALF_MS) {
        cp += SIXTEEN;
      }
    }
    uint64_t off, cps;
    if (!to_samples(t_occ, srate, off) || !to_samples(cp, srate, cps)) {
      return fail(SRS_AMD_EINVAL, "Incompatible sampling rate %u Hz with the occasion timing.", srate);
    }
    g.sample_offset[i]  = static_cast<uint32_t>(off);
    g.cp_samples[i]     = static_cast<uint32_t>(cps);
    g.min_input_samples = std::max<uint64_t>(g.min_input_samples,
                                             off + cps + static_cast<uint64_t>(g.nof_symbols) * g.dft_size);
  }

  // get_prach_window_duration
  {
    const uint64_t psd     = is_long ? 2192u : symbol;
    uint64_t       t_start = psd * c.start_symbol;
    if (t_start > 0) {
      t_start += SIXTEEN;
    }
    if (t_start > HALF_MS) {
      t_start += SIXTEEN;
    }
    uint64_t t_end;
    if (!is_long) {
      t_end = t_start + psd * f.duration * c.nof_td_occasions;
      if (t_start == 0) {
        t_end += SIXTEEN;
      }
      if (t_start <= HALF_MS && t_end > HALF_MS) {
        t_end += SIXTEEN;
      }
    } else {
      // rounded up to a whole subframe, through seconds as the reference does
      const double T_C     = 1.0 / (480000.0 * 4096.0);
      const double seconds = static_cast<double>((t_start + f.cp + sym_len) * 64) * T_C;
      t_end                = static_cast<uint64_t>(std::ceil(seconds * 1e3)) * 30720u;
    }
    if (!to_samples(t_end, srate, g.window_samples)) {
      return fail(SRS_AMD_EINVAL, "Incompatible sampling rate %u Hz with the window duration.", srate);
    }
  }
  g.nof_elements = static_cast<uint64_t>(c.nof_td_occasions) * c.nof_fd_occasions * c.nof_ports * g.nof_symbols * g.L_ra;
  return SRS_AMD_OK;
}

// W_n^m = exp(-2*pi*i*m/n), double precision rounded to float (dft_engine.h).
std::vector<float2> twiddle_table(uint32_t n)
{
  std::vector<float2> t(n);
  for (uint32_t m = 0; m != n; ++m) {
    const double a = -2.0 * M_PI * static_cast<double>(m) / static_cast<double>(n);
    t[m]           = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
  }
  return t;
}

} // namespace

struct srs_amd_prach_demodulator {
  int                         device = 0;
  uint32_t                    srate  = 0;
  hipStream_t                 stream = nullptr; // host form
  std::map<uint32_t, float2*> twiddles;         // by table size: every M and every split N of this sampling rate
  device_buffer               descriptors;
  device_buffer               partials;
  device_buffer               host_io;
  pinned_stage                stage;
  stream_order                order;
  std::mutex                  mtx;
  std::mutex                  host_mtx;

  ~srs_amd_prach_demodulator()
  {
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    for (auto& t : twiddles) {
      (void)hipFree(t.second);
    }
  }

  hipError_t add_table(uint32_t n)
  {
    if (twiddles.count(n) != 0) {
      return hipSuccess;
    }
    const std::vector<float2> t = twiddle_table(n);
    float2*                   p = nullptr;
    hipError_t                e = hipMalloc(reinterpret_cast<void**>(&p), t.size() * sizeof(float2));
    if (e == hipSuccess) {
      twiddles[n] = p;
      e           = hipMemcpy(p, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
    }
    return e;
  }
};

extern "C" {

int srs_amd_prach_demod_get_geometry(uint32_t                          srate_hz,
                                     const srs_amd_prach_demod_config* config,
                                     srs_amd_prach_demod_geometry*     geometry)
{
  if (config == nullptr || geometry == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived   d{};
  const int rc = derive(srate_hz, *config, d);
  if (rc == SRS_AMD_OK) {
    *geometry = d.g;
  }
  return rc;
}

int srs_amd_prach_demod_get_detector_offsets(uint32_t                          srate_hz,
                                             const srs_amd_prach_demod_config* config,
                                             uint64_t                          out_offset,
                                             uint64_t*                         offsets)
{
  if (config == nullptr || offsets == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived   d{};
  const int rc = derive(srate_hz, *config, d);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  const uint64_t occasion = static_cast<uint64_t>(config->nof_ports) * d.g.nof_symbols * d.g.L_ra;
  for (uint32_t i = 0; i != config->nof_td_occasions * config->nof_fd_occasions; ++i) {
    offsets[i] = out_offset + i * occasion;
  }
  return SRS_AMD_OK;
}

int srs_amd_prach_demodulator_create(srs_amd_prach_demodulator** dem, uint32_t srate_hz, int device)
{
  if (dem == nullptr) {
    return fail(SRS_AMD_EINVAL, "null handle pointer");
  }
  *dem = nullptr;
  if (!srate_supported(srate_hz)) {
    return fail(SRS_AMD_EINVAL, "Unsupported sampling rate %u Hz.", srate_hz);
  }
  int rc = select_device(device);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  auto* d      = new srs_amd_prach_demodulator();
  d->device    = device;
  d->srate     = srate_hz;
  hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
  for (uint32_t ra_hz : {1250u, 5000u, 15000u, 30000u, 60000u, 120000u}) {
    uint32_t M = 0, D = 0;
    if (e != hipSuccess || srate_hz % ra_hz != 0 || !dft_plan(srate_hz / ra_hz, M, D)) {
      continue;
    }
    e = d->add_table(M);
    if (e == hipSuccess && D != 1) {
      e = d->add_table(srate_hz / ra_hz);
    }
  }
  if (e != hipSuccess) {
    delete d;
    return hip_fail(e, "PRACH demodulator tables");
  }
  *dem = d;
  return SRS_AMD_OK;
}

void srs_amd_prach_demodulator_destroy(srs_amd_prach_demodulator* dem)
{
  delete dem;
}

int srs_amd_prach_demodulate_batch(srs_amd_prach_demodulator*        dem,
                                   const srs_amd_prach_demod_config* configs,
                                   uint32_t                          nof_windows,
                                   const void*                       d_samples,
                                   const uint64_t*                   sample_offsets,
                                   const uint64_t*                   port_strides,
                                   const uint64_t*                   nof_samples,
                                   void*                             d_out,
                                   const uint64_t*                   out_offsets,
                                   void*                             stream)
{
  if (dem == nullptr) {
    return fail(SRS_AMD_EINVAL, "null PRACH demodulator");
  }
  if (nof_windows == 0) {
    return SRS_AMD_OK;
  }
  if (configs == nullptr || d_samples == nullptr || sample_offsets == nullptr || port_strides == nullptr ||
      nof_samples == nullptr || d_out == nullptr || out_offsets == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  if ((reinterpret_cast<uintptr_t>(d_samples) & 7u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 3u) != 0) {
    return fail(SRS_AMD_EINVAL, "misaligned device buffer");
  }
  // validate every window before anything is launched
  std::vector<derived> geo(nof_windows);
  for (uint32_t i = 0; i != nof_windows; ++i) {
    const int rc = derive(dem->srate, configs[i], geo[i]);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    if (nof_samples[i] < geo[i].g.min_input_samples) {
      return fail(SRS_AMD_EINVAL,
                  "The number of input samples (i.e., %llu) must be equal to or greater than what the occasions read "
                  "(i.e., %llu).",
                  static_cast<unsigned long long>(nof_samples[i]),
                  static_cast<unsigned long long>(geo[i].g.min_input_samples));
    }
    if (port_strides[i] < nof_samples[i]) {
      return fail(SRS_AMD_EINVAL, "The port stride (i.e., %llu) is below the number of samples (i.e., %llu).",
                  static_cast<unsigned long long>(port_strides[i]), static_cast<unsigned long long>(nof_samples[i]));
    }
  }

  // windows, and per launch one item per workgroup
  std::vector<prach_demod_window> win(nof_windows);
  size_t                          partial_values = 0;
  for (uint32_t i = 0; i != nof_windows; ++i) {
    const srs_amd_prach_demod_config&   c = configs[i];
    const srs_amd_prach_demod_geometry& g = geo[i].g;
    prach_demod_window&                 w = win[i];
    std::memset(&w, 0, sizeof(w));
    w.in          = static_cast<const float2*>(d_samples) + sample_offsets[i];
    w.out         = static_cast<uint32_t*>(d_out) + out_offsets[i];
    w.twiddles    = dem->twiddles.at(g.sub_dft_size);
    w.port_stride = port_strides[i];
    w.N           = g.dft_size;
    w.M           = g.sub_dft_size;
    w.D           = g.nof_sub_dfts;
    w.A           = 1;
    w.nof_ports   = c.nof_ports;
    w.nof_td      = c.nof_td_occasions;
    w.nof_fd      = c.nof_fd_occasions;
    w.nof_symbols = g.nof_symbols;
    w.L_ra        = g.L_ra;
    w.k0          = g.k_start[0];
    w.k_step      = geo[i].k_step;
    w.half        = geo[i].half;
    w.scale       = 1.0F / std::sqrt(g.dft_size); // as the reference: float / double, rounded to float
    for (uint32_t t = 0; t != c.nof_td_occasions; ++t) {
      w.first[t] = g.sample_offset[t] + g.cp_samples[t];
    }
    if (w.D != 1) {
      w.A          = residues_per_group(w.D);
      w.twiddles_n = dem->twiddles.at(w.N);
      // the offset in values for now; the pointer once the scratch is in place
      w.partial = reinterpret_cast<float2*>(partial_values);
      partial_values += static_cast<size_t>(c.nof_ports) * c.nof_td_occasions * g.nof_symbols * (w.D / w.A) * c.nof_fd_occasions *
                        g.L_ra;
    }
  }
  struct launch {
    uint32_t size; // N (planned) or M (split); 0: finish
    bool     split;
    uint32_t begin, count;
  };
  std::vector<launch>           launches;
  std::vector<prach_demod_item> items;
  auto add_items = [&](uint32_t size, bool split, bool finish) {
    const uint32_t begin = static_cast<uint32_t>(items.size());
    for (uint32_t i = 0; i != nof_windows; ++i) {
      const prach_demod_window& w = win[i];
      const bool mine = finish ? w.D != 1 : (split ? w.D != 1 && w.M == size : w.D == 1 && w.N == size);
      if (!mine) {
        continue;
      }
      // The groups of a symbol read interleaved runs of the same cache lines.  Workgroups go to the eight XCDs in
      // turn, so the symbols are taken eight at a time with the group index outermost: workgroup 8 q + j of such a
      // block is group q of its symbol j, and all groups of a symbol meet in one XCD's L2.
      const uint32_t groups = split ? w.D / w.A : 1;
      const uint32_t per_port = w.nof_td * w.nof_symbols, symbols = w.nof_ports * per_port;
      for (uint32_t first = 0; first < symbols; first += 8) {
        const uint32_t block = std::min(8u, symbols - first);
        for (uint32_t q = 0; q != groups; ++q) {
          for (uint32_t j = first; j != first + block; ++j) {
            items.push_back({i, static_cast<uint8_t>(j / per_port), static_cast<uint8_t>(j % per_port / w.nof_symbols),
                             static_cast<uint8_t>(j % w.nof_symbols), static_cast<uint8_t>(q)});
          }
        }
      }
    }
    if (items.size() != begin) {
      launches.push_back({size, split, begin, static_cast<uint32_t>(items.size()) - begin});
    }
  };
  std::vector<uint32_t> seen;
  for (const prach_demod_window& w : win) {
    if (w.D == 1 && std::find(seen.begin(), seen.end(), w.N) == seen.end()) {
      seen.push_back(w.N);
      add_items(w.N, false, false);
    }
  }
#define SRS_SUB(MM) add_items(MM, true, false);
  SRS_PRACH_DEMOD_FOR_EACH_SUB(SRS_SUB)
#undef SRS_SUB
  add_items(0, false, true);
  if (items.size() > 0x7fffffffu) {
    return fail(SRS_AMD_EINVAL, "Too many symbols in one batch.");
  }

  hipStream_t                 s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(dem->mtx);
  hipError_t                  e = hipSetDevice(dem->device);
  if (e == hipSuccess && partial_values != 0) {
    e = dem->partials.ensure(partial_values * sizeof(float2));
  }
  if (e != hipSuccess) {
    return hip_fail(e, "PRACH demodulator scratch");
  }
  for (prach_demod_window& w : win) {
    if (w.D != 1) {
      w.partial = dem->partials.as<float2>() + reinterpret_cast<size_t>(w.partial);
    }
  }
  const size_t win_bytes = align_up(win.size() * sizeof(prach_demod_window), 16);
  const size_t bytes     = win_bytes + items.size() * sizeof(prach_demod_item);
  staged_call  call("PRACH demodulator", staged_call::DEVICE_IS_CURRENT, dem->descriptors, bytes, dem->stage, bytes,
                    dem->order, s);
  if (!call.ok()) {
    return call.finish();
  }
  std::memcpy(call.host(), win.data(), win.size() * sizeof(prach_demod_window));
  std::memcpy(call.host(win_bytes), items.data(), items.size() * sizeof(prach_demod_item));
  e = call.upload(dem->descriptors.ptr, bytes);
  const auto* d_win   = dem->descriptors.as<prach_demod_window>();
  const auto* d_items = reinterpret_cast<const prach_demod_item*>(dem->descriptors.as<uint8_t>() + win_bytes);
  for (size_t k = 0; k != launches.size() && e == hipSuccess; ++k) {
    const launch& l = launches[k];
    if (l.size == 0) {
      e = launch_prach_demod_finish(d_win, d_items + l.begin, l.count, s);
    } else if (l.split) {
      e = launch_prach_demod_split(d_win, d_items + l.begin, l.count, l.size, s);
    } else {
      e = launch_prach_demod_planned(d_win, d_items + l.begin, l.count, l.size, s);
    }
  }
  return call.finish(e);
}

int srs_amd_prach_demodulate(srs_amd_prach_demodulator*        dem,
                             const srs_amd_prach_demod_config* config,
                             const float*                      samples,
                             uint64_t                          nof_samples,
                             uint64_t                          port_stride,
                             void*                             out)
{
  if (dem == nullptr || config == nullptr || samples == nullptr || out == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  int     rc = derive(dem->srate, *config, d);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  if (nof_samples < d.g.min_input_samples || port_stride < nof_samples) {
    return fail(SRS_AMD_EINVAL, "The input (%llu samples, port stride %llu) is shorter than what the occasions read "
                "(i.e., %llu).", static_cast<unsigned long long>(nof_samples),
                static_cast<unsigned long long>(port_stride), static_cast<unsigned long long>(d.g.min_input_samples));
  }
  // only what the occasions read travels, the ports back to back
  const uint64_t used     = d.g.min_input_samples;
  const size_t   in_bytes = static_cast<size_t>(config->nof_ports) * used * sizeof(float2);
  const size_t   out_off  = align_up(in_bytes, 16);
  const size_t   out_bytes = d.g.nof_elements * sizeof(uint32_t);
  host_call      call("PRACH demodulator", dem->host_mtx, dem->device, dem->stream);
  call.grow(dem->host_io, out_off + out_bytes);
  for (uint32_t p = 0; p != config->nof_ports; ++p) {
    call.in(dem->host_io.as<uint8_t>() + p * used * sizeof(float2), samples + 2 * p * port_stride,
            used * sizeof(float2));
  }
  if (!call.ok()) {
    return call.finish();
  }
  const uint64_t zero = 0;
  rc = srs_amd_prach_demodulate_batch(dem, config, 1, dem->host_io.ptr, &zero, &used, &used,
                                      dem->host_io.as<uint8_t>() + out_off, &zero, dem->stream);
  if (rc == SRS_AMD_OK) {
    call.out(out, dem->host_io.as<uint8_t>() + out_off, out_bytes);
  }
  return call.finish(rc);
}

} // extern "C"
