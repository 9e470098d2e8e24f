// prach_golden_gen.cpp -- writes tests/golden/prach_golden.npz: seeded PRACH occasions and what the reference's
// generic PRACH detector reports for them.
//
// NEEDS THE REFERENCE TREE (srsRAN Project): it is compiled together with the reference's own sources
//   lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp, prach_detector_generic_thresholds.cpp,
//   prach_detector_phy_validator_impl.cpp, prach_generator_impl.cpp,
//   lib/phy/generic_functions/dft_processor_generic_impl.cpp, lib/ran/prach/prach_cyclic_shifts.cpp,
//   lib/ran/prach/prach_preamble_information.cpp and lib/srsvec/*.cpp
// with the flags of oracle/Makefile (CXXFLAGS_REF), e.g. from a directory outside this repository:
//   g++ -std=c++17 -O3 -DFMT_HEADER_ONLY -I$REF/include -I$REF/external/fmt/include -I$REF/external -I$REF/lib \
//       -march=x86-64-v3 -w <repo>/tools/prach_golden_gen.cpp <the sources above> -o prach_golden_gen
//   ./prach_golden_gen <repo>/tests/golden/prach_golden.npz
// It is run by no test, bench or build: the .npz it wrote is committed, and the tests read only that file.
//
// Every case: 0..3 preambles of the case's configuration (the reference's own generator), each delayed by a whole
// number of IDFT samples below 0.8 max_delay, a random phase per port, complex Gaussian noise, the sum rounded to
// bf16.  The threshold and the window margin are the ones the reference looked up; they are recorded per case
// because the product takes both as inputs.
//
// Arrays of the .npz (NN = case number, two digits):
//   names             uint8   the case names joined by '\n'
//   roots_long        int32   [838] physical root u of every logical long root index (TS 38.211 Table 6.3.3.1-3),
//   roots_short       int32   [138] ... and short (Table 6.3.3.1-4), recovered from the generated sequences
//   ref_detect_us     float64 [2] single-thread time of one reference detect() call, microseconds: format 0 ZCZ 0
//                             4 ports, format B4 ZCZ 0 30 kHz 4 ports (informative)
//   cNN_cfg           int32   [format, ra_scs, root_sequence_index, zero_correlation_zone, start_preamble_index,
//                              nof_preamble_indices, nof_rx_ports, combine_symbols, idft_size, validator_accepts]
//                             format: 0..3, then A1 A2 A3 B1 B4 C0 C2 A1/B1 A2/B2 A3/B3 = 4..13
//                             ra_scs: 0 = 15, 1 = 30, 2 = 60, 3 = 120, 4 = 1.25, 5 = 5 kHz
//   cNN_geo           int32   [L_ra, N_cs, nof_shifts, nof_sequences, win_width, max_delay_samples, nof_symbols,
//                              win_margin]
//   cNN_thr           float32 [threshold]
//   cNN_x             uint16  [ports, symbols, L_ra, 2] cbf16 bit patterns (re, im)
//   cNN_tx            int32   [n, 2] transmitted (preamble index, delay in IDFT samples)
//   cNN_res           float64 [rssi_dB, time_resolution s, time_advance_max s]
//   cNN_det           float64 [n, 4] detected (preamble_index, time_advance s, detection_metric, preamble_power_dB)
#include "phy/generic_functions/dft_processor_generic_impl.h"
#include "phy/upper/channel_processors/prach_detector_generic_impl.h"
#include "phy/upper/channel_processors/prach_detector_generic_thresholds.h"
#include "phy/upper/channel_processors/prach_generator_impl.h"
#include "srsran/phy/support/prach_buffer.h"
#include "srsran/phy/upper/channel_processors/prach_detector_phy_validator.h"
#include "srsran/ran/prach/prach_cyclic_shifts.h"
#include "srsran/ran/prach/prach_preamble_information.h"

#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

using namespace srsran;

namespace {

// ---- a stored (uncompressed) .npz ------------------------------------------------------------------------------
uint32_t crc32_of(const std::vector<uint8_t>& d)
{
  static uint32_t table[256];
  static bool     init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) {
        c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      }
      table[i] = c;
    }
    init = true;
  }
  uint32_t c = 0xFFFFFFFFu;
  for (uint8_t b : d) {
    c = table[(c ^ b) & 0xFF] ^ (c >> 8);
  }
  return c ^ 0xFFFFFFFFu;
}

struct npz_writer {
  struct entry {
    std::string name;
    uint32_t    crc, size, offset;
  };
  std::vector<uint8_t> out;
  std::vector<entry>   entries;

  void u16(uint16_t v) { out.push_back(v & 0xFF), out.push_back(v >> 8); }
  void u32(uint32_t v) { u16(v & 0xFFFF), u16(v >> 16); }

  void add(const std::string& key, const char* descr, const std::vector<size_t>& shape, const void* data, size_t bytes)
  {
    std::string shp = "(";
    for (size_t i = 0; i < shape.size(); ++i) {
      shp += std::to_string(shape[i]) + (shape.size() == 1 || i + 1 < shape.size() ? "," : "");
    }
    shp += ")";
    std::string hdr = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shp + ", }";
    while ((10 + hdr.size() + 1) % 64 != 0) {
      hdr += ' ';
    }
    hdr += '\n';
    std::vector<uint8_t> f = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, uint8_t(hdr.size() & 0xFF), uint8_t(hdr.size() >> 8)};
    f.insert(f.end(), hdr.begin(), hdr.end());
    const auto* p = static_cast<const uint8_t*>(data);
    f.insert(f.end(), p, p + bytes);
    entry e{key + ".npy", crc32_of(f), uint32_t(f.size()), uint32_t(out.size())};
    u32(0x04034b50), u16(20), u16(0), u16(0), u16(0), u16(0x21), u32(e.crc), u32(e.size), u32(e.size);
    u16(e.name.size()), u16(0);
    out.insert(out.end(), e.name.begin(), e.name.end());
    out.insert(out.end(), f.begin(), f.end());
    entries.push_back(e);
  }
  template <typename T>
  void add(const std::string& key, const std::vector<T>& v, std::vector<size_t> shape = {})
  {
    const char* descr = std::is_same<T, double>::value    ? "<f8"
                        : std::is_same<T, float>::value   ? "<f4"
                        : std::is_same<T, int32_t>::value ? "<i4"
                        : std::is_same<T, uint16_t>::value ? "<u2"
                                                           : "|u1";
    if (shape.empty()) {
      shape = {v.size()};
    }
    add(key, descr, shape, v.data(), v.size() * sizeof(T));
  }
  bool save(const char* path)
  {
    const uint32_t cd = out.size();
    for (const entry& e : entries) {
      u32(0x02014b50), u16(20), u16(20), u16(0), u16(0), u16(0), u16(0x21), u32(e.crc), u32(e.size), u32(e.size);
      u16(e.name.size()), u16(0), u16(0), u16(0), u16(0), u32(0), u32(e.offset);
      out.insert(out.end(), e.name.begin(), e.name.end());
    }
    const uint32_t cd_size = out.size() - cd;
    u32(0x06054b50), u16(0), u16(0), u16(entries.size()), u16(entries.size()), u32(cd_size), u32(cd), u16(0);
    FILE* f = std::fopen(path, "wb");
    if (f == nullptr) {
      return false;
    }
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok;
  }
};

// ---- a PRACH buffer of one occasion ----------------------------------------------------------------------------
class occasion_buffer : public prach_buffer
{
public:
  occasion_buffer(unsigned ports_, unsigned symbols_, unsigned L_) :
    ports(ports_), symbols(symbols_), L(L_), data(size_t(ports_) * symbols_ * L_)
  {
  }
  unsigned      get_max_nof_ports() const override { return ports; }
  unsigned      get_max_nof_td_occasions() const override { return 1; }
  unsigned      get_max_nof_fd_occasions() const override { return 1; }
  unsigned      get_max_nof_symbols() const override { return symbols; }
  unsigned      get_sequence_length() const override { return L; }
  span<cbf16_t> get_symbol(unsigned p, unsigned, unsigned, unsigned s) override
  {
    return span<cbf16_t>(data).subspan((size_t(p) * symbols + s) * L, L);
  }
  span<const cbf16_t> get_symbol(unsigned p, unsigned, unsigned, unsigned s) const override
  {
    return span<const cbf16_t>(data).subspan((size_t(p) * symbols + s) * L, L);
  }
  unsigned             ports, symbols, L;
  std::vector<cbf16_t> data;
};

struct tx_preamble {
  unsigned index;
  double   delay_fraction; // of 0.8 max_delay; rounded down to a whole IDFT sample
};

struct test_case {
  const char*              name;
  prach_format_type        format;
  prach_subcarrier_spacing scs;
  unsigned                 root_sequence_index, zcz, start, nof, ports;
  bool                     combine;
  std::vector<tx_preamble> tx;
  double                   amplitude, noise_sigma; // per subcarrier; both 0: an all-zero buffer
  uint64_t                 seed;
};

struct geometry {
  unsigned L_ra, N_cs, nof_shifts, nof_sequences, win_width, max_delay, nof_symbols, idft_size;
};

// the geometry derived at the top of prach_detector_generic_impl::detect, from the reference's own tables
geometry derive(const test_case& c, unsigned idft_long, unsigned idft_short)
{
  geometry                   g{};
  const bool                 lng  = is_long_preamble(c.format);
  prach_preamble_information info = lng ? get_prach_preamble_long_info(c.format)
                                        : get_prach_preamble_short_info(c.format, c.scs, false);
  g.N_cs          = prach_cyclic_shifts_get(c.scs, restricted_set_config::UNRESTRICTED, c.zcz);
  g.L_ra          = lng ? 839 : 139;
  g.nof_shifts    = 1;
  g.nof_sequences = 64;
  if (g.N_cs != 0) {
    g.nof_shifts    = std::min(64U, g.L_ra / g.N_cs);
    g.nof_sequences = (64 + g.nof_shifts - 1) / g.nof_shifts;
  }
  g.idft_size       = lng ? idft_long : idft_short;
  double   cp       = info.cp_length.to_seconds();
  unsigned cp_prach = static_cast<unsigned>(std::floor(cp * g.L_ra * ra_scs_to_Hz(info.scs)));
  unsigned w        = g.N_cs == 0 ? cp_prach : std::min(g.N_cs, cp_prach);
  g.win_width       = (w * g.idft_size) / g.L_ra;
  unsigned md       = g.N_cs == 0 ? cp_prach : std::min(std::max(g.N_cs, 1U) - 1U, cp_prach);
  g.max_delay       = (md * g.idft_size) / g.L_ra;
  g.nof_symbols     = info.nof_symbols;
  return g;
}

std::unique_ptr<prach_detector_generic_impl> make_detector(unsigned idft_long, unsigned idft_short, bool combine)
{
  dft_processor::configuration cl{idft_long, dft_processor::direction::INVERSE};
  dft_processor::configuration cs{idft_short, dft_processor::direction::INVERSE};
  return std::make_unique<prach_detector_generic_impl>(std::make_unique<dft_processor_generic_impl>(cl),
                                                       std::make_unique<dft_processor_generic_impl>(cs),
                                                       std::make_unique<prach_generator_impl>(),
                                                       combine);
}

double gauss(std::mt19937_64& rng)
{
  // Box-Muller on the generator's raw output (the standard fixes mt19937_64, not the distributions)
  const double u1 = (double(rng() >> 11) + 1.0) / 9007199254740993.0;
  const double u2 = double(rng() >> 11) / 9007199254740992.0;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
}

void fill(occasion_buffer& buf, const test_case& c, const geometry& g, std::vector<int32_t>& tx_out)
{
  std::mt19937_64                        rng(c.seed);
  prach_generator_impl                   gen;
  std::vector<std::complex<double>>      sum(size_t(buf.ports) * buf.symbols * g.L_ra);
  for (const tx_preamble& t : c.tx) {
    prach_generator::configuration gc{};
    gc.format                = c.format;
    gc.root_sequence_index   = c.root_sequence_index;
    gc.preamble_index        = t.index;
    gc.restricted_set        = restricted_set_config::UNRESTRICTED;
    gc.zero_correlation_zone = c.zcz;
    span<const cf_t> y       = gen.generate(gc);
    const unsigned   delay   = static_cast<unsigned>(std::floor(t.delay_fraction * 0.8 * g.max_delay));
    tx_out.push_back(t.index);
    tx_out.push_back(delay);
    for (unsigned p = 0; p != buf.ports; ++p) {
      const double phase = 2.0 * M_PI * double(rng() >> 11) / 9007199254740992.0;
      for (unsigned s = 0; s != buf.symbols; ++s) {
        for (unsigned k = 0; k != g.L_ra; ++k) {
          // subcarrier k of the buffer is frequency k - L_ra / 2 of the detector's IDFT
          const double a = phase - 2.0 * M_PI * (double(k) - double(g.L_ra / 2)) * delay / g.idft_size;
          sum[(size_t(p) * buf.symbols + s) * g.L_ra + k] +=
              std::complex<double>(y[k].real(), y[k].imag()) * std::polar(c.amplitude / std::sqrt(double(g.L_ra)), a);
        }
      }
    }
  }
  for (size_t i = 0; i != sum.size(); ++i) {
    if (c.noise_sigma > 0) {
      sum[i] += std::complex<double>(gauss(rng), gauss(rng)) * (c.noise_sigma / std::sqrt(2.0));
    }
    buf.data[i] = cbf16_t(cf_t(float(sum[i].real()), float(sum[i].imag())));
  }
}

// physical root of a frequency-domain sequence y_u: its inverse transform is x_u(n) = exp(-j pi u n (n + 1) / L), so
// x_u(1) / x_u(0) = exp(-j 2 pi u / L)
unsigned root_of(span<const cf_t> y)
{
  const unsigned       L = y.size();
  std::complex<double> x0 = 0, x1 = 0;
  for (unsigned k = 0; k != L; ++k) {
    std::complex<double> v(y[k].real(), y[k].imag());
    x0 += v;
    x1 += v * std::polar(1.0, 2.0 * M_PI * k / L);
  }
  const double step = -std::arg(x1 / x0) * L / (2.0 * M_PI);
  return unsigned(std::lround(step) + L) % L;
}

double time_detect(const test_case& c)
{
  geometry             g = derive(c, 1024, 256);
  occasion_buffer      buf(c.ports, g.nof_symbols, g.L_ra);
  std::vector<int32_t> tx;
  fill(buf, c, g, tx);
  auto                          det = make_detector(1024, 256, true);
  prach_detector::configuration cfg{};
  cfg.root_sequence_index   = c.root_sequence_index;
  cfg.format                = c.format;
  cfg.restricted_set        = restricted_set_config::UNRESTRICTED;
  cfg.zero_correlation_zone = c.zcz;
  cfg.start_preamble_index  = c.start;
  cfg.nof_preamble_indices  = c.nof;
  cfg.ra_scs                = c.scs;
  cfg.nof_rx_ports          = c.ports;
  volatile float sink       = 0;
  for (int i = 0; i < 3; ++i) {
    sink = sink + det->detect(buf, cfg).rssi_dB;
  }
  const int  reps = 50;
  const auto t0   = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) {
    sink = sink + det->detect(buf, cfg).rssi_dB;
  }
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <out.npz>\n", argv[0]);
    return 2;
  }
  using F   = prach_format_type;
  using S   = prach_subcarrier_spacing;
  const std::vector<test_case> cases = {
      {"f0_zcz0_1port", F::zero, S::kHz1_25, 22, 0, 0, 64, 1, true, {{5, 0.31}, {40, 0.77}}, 1.0, 1.0, 101},
      {"f0_zcz1_2ports", F::zero, S::kHz1_25, 100, 1, 0, 64, 2, true, {{0, 0.5}, {63, 0.2}}, 1.0, 1.0, 102},
      {"f0_zcz12_4ports", F::zero, S::kHz1_25, 836, 12, 0, 64, 4, true, {{6, 0.9}, {63, 0.1}}, 1.0, 1.0, 103},
      {"f1_zcz6_2ports", F::one, S::kHz1_25, 7, 6, 0, 64, 2, true, {{17, 0.6}}, 1.0, 1.0, 104},
      {"f3_5khz_zcz8_2ports", F::three, S::kHz5, 411, 8, 0, 64, 2, true, {{33, 0.45}, {2, 0.05}}, 1.0, 1.0, 105},
      {"f0_zcz9_range10_20", F::zero, S::kHz1_25, 300, 9, 10, 20, 2, true, {{12, 0.3}, {29, 0.7}, {45, 0.5}}, 1.0, 1.0, 106},
      {"b4_30khz_zcz0_2ports", F::B4, S::kHz30, 17, 0, 0, 64, 2, true, {{9, 0.4}}, 1.0, 1.0, 107},
      {"b4_30khz_zcz10_1port", F::B4, S::kHz30, 130, 10, 0, 64, 1, true, {{20, 0.5}, {21, 0.25}}, 1.0, 1.0, 108},
      {"a1_15khz_zcz8_2ports", F::A1, S::kHz15, 60, 8, 0, 64, 2, true, {{3, 0.3}, {50, 0.6}}, 1.0, 0.7, 109},
      {"c0_15khz_zcz9_1port", F::C0, S::kHz15, 1, 9, 0, 64, 1, true, {{8, 0.5}}, 1.0, 0.5, 110},
      {"c0_15khz_zcz9_2ports", F::C0, S::kHz15, 90, 9, 0, 64, 2, true, {{31, 0.35}}, 1.0, 0.5, 111},
      {"a2_30khz_zcz11_2ports_nocombine", F::A2, S::kHz30, 45, 11, 0, 64, 2, false, {{11, 0.5}, {12, 0.15}}, 1.0, 0.7, 112},
      {"f0_zcz8_noise_only", F::zero, S::kHz1_25, 500, 8, 0, 64, 2, true, {}, 0.0, 1.0, 113},
      {"f0_zcz5_all_zero", F::zero, S::kHz1_25, 3, 5, 0, 64, 1, true, {}, 0.0, 0.0, 114},
      {"f0_zcz11_three_preambles", F::zero, S::kHz1_25, 700, 11, 0, 64, 4, true, {{1, 0.2}, {7, 0.8}, {13, 0.5}}, 1.0, 1.0, 115},
  };

  npz_writer  npz;
  std::string names;
  for (size_t i = 0; i != cases.size(); ++i) {
    const test_case& c = cases[i];
    names += (i ? "\n" : "") + std::string(c.name);
    const geometry       g = derive(c, 1024, 256);
    occasion_buffer      buf(c.ports, g.nof_symbols, g.L_ra);
    std::vector<int32_t> tx;
    fill(buf, c, g, tx);

    detail::threshold_params tp;
    tp.nof_rx_ports          = c.ports;
    tp.scs                   = c.scs;
    tp.format                = c.format;
    tp.zero_correlation_zone = c.zcz;
    tp.combine_symbols       = c.combine;
    const auto th            = detail::get_threshold_and_margin(tp);
    const bool accepted      = validate_prach_detector_phy(c.format, c.scs, c.zcz, c.ports).has_value();

    prach_detector::configuration cfg{};
    cfg.root_sequence_index   = c.root_sequence_index;
    cfg.format                = c.format;
    cfg.restricted_set        = restricted_set_config::UNRESTRICTED;
    cfg.zero_correlation_zone = c.zcz;
    cfg.start_preamble_index  = c.start;
    cfg.nof_preamble_indices  = c.nof;
    cfg.ra_scs                = c.scs;
    cfg.nof_rx_ports          = c.ports;
    auto                   det = make_detector(1024, 256, c.combine);
    prach_detection_result res = det->detect(buf, cfg);

    char key[16];
    std::snprintf(key, sizeof(key), "c%02zu_", i);
    const std::string k = key;
    npz.add<int32_t>(k + "cfg", {int32_t(c.format), int32_t(c.scs), int32_t(c.root_sequence_index), int32_t(c.zcz),
                                 int32_t(c.start), int32_t(c.nof), int32_t(c.ports), int32_t(c.combine),
                                 int32_t(g.idft_size), int32_t(accepted)});
    npz.add<int32_t>(k + "geo", {int32_t(g.L_ra), int32_t(g.N_cs), int32_t(g.nof_shifts), int32_t(g.nof_sequences),
                                 int32_t(g.win_width), int32_t(g.max_delay), int32_t(g.nof_symbols), int32_t(th.second)});
    npz.add<float>(k + "thr", {th.first});
    std::vector<uint16_t> x(buf.data.size() * 2);
    std::memcpy(x.data(), buf.data.data(), x.size() * sizeof(uint16_t));
    static_assert(sizeof(cbf16_t) == 4, "cbf16_t is two 16-bit halves");
    npz.add<uint16_t>(k + "x", x, {c.ports, g.nof_symbols, g.L_ra, 2});
    npz.add<int32_t>(k + "tx", tx, {tx.size() / 2, 2});
    npz.add<double>(k + "res", {double(res.rssi_dB), res.time_resolution.to_seconds(), res.time_advance_max.to_seconds()});
    std::vector<double> d;
    for (const auto& p : res.preambles) {
      d.insert(d.end(), {double(p.preamble_index), p.time_advance.to_seconds(), double(p.detection_metric),
                         double(p.preamble_power_dB)});
    }
    npz.add<double>(k + "det", d, {d.size() / 4, 4});
    std::printf("%-34s thr %.3f margin %2u %s win %3u maxd %3u  rssi %7.2f dB  detected:", c.name, th.first, th.second,
                accepted ? "ok " : "RED", g.win_width, g.max_delay, res.rssi_dB);
    for (const auto& p : res.preambles) {
      std::printf(" %u@%.0f(m %.2f, %.1f dB)", p.preamble_index,
                  p.time_advance.to_seconds() / res.time_resolution.to_seconds(), p.detection_metric, p.preamble_power_dB);
    }
    std::printf("   sent:");
    for (size_t j = 0; j < tx.size(); j += 2) {
      std::printf(" %d@%d", tx[j], tx[j + 1]);
    }
    std::printf("\n");
  }
  npz.add<uint8_t>("names", std::vector<uint8_t>(names.begin(), names.end()));

  prach_generator_impl gen;
  std::vector<int32_t> roots_long, roots_short;
  for (unsigned i = 0; i != 838 + 138; ++i) {
    prach_generator::configuration gc{};
    gc.format                = i < 838 ? F::zero : F::A1;
    gc.root_sequence_index   = i < 838 ? i : i - 838;
    gc.preamble_index        = 0;
    gc.restricted_set        = restricted_set_config::UNRESTRICTED;
    gc.zero_correlation_zone = 0;
    (i < 838 ? roots_long : roots_short).push_back(root_of(gen.generate(gc)));
  }
  npz.add<int32_t>("roots_long", roots_long);
  npz.add<int32_t>("roots_short", roots_short);

  const test_case t0 = {"time_f0", F::zero, S::kHz1_25, 1, 0, 0, 64, 4, true, {{5, 0.3}}, 1.0, 1.0, 1};
  const test_case t1 = {"time_b4", F::B4, S::kHz30, 1, 0, 0, 64, 4, true, {{5, 0.3}}, 1.0, 1.0, 2};
  const double    us0 = time_detect(t0), us1 = time_detect(t1);
  std::printf("reference detect(), one thread: format 0 ZCZ 0 4 ports %.1f us, format B4 ZCZ 0 30 kHz 4 ports %.1f us\n",
              us0, us1);
  npz.add<double>("ref_detect_us", {us0, us1});
  if (!npz.save(argv[1])) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  return 0;
}
