// srs_golden_gen.cpp -- writes tests/golden/srs_golden.npz: seeded SRS receptions and what the reference's generic
// SRS estimator reports for them.
//
// NEEDS THE REFERENCE TREE (srsRAN Project): it is compiled together with the reference's own sources
//   lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp, srs_validator_generic_impl.cpp,
//   lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp,
//   lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.cpp,
//   lib/phy/generic_functions/dft_processor_generic_impl.cpp, lib/ran/srs/srs_information.cpp,
//   lib/ran/srs/srs_bandwidth_configuration.cpp, lib/support/math_utils.cpp and lib/srsvec/*.cpp
// with the flags of oracle/Makefile (CXXFLAGS_REF), e.g. from a directory outside this repository:
//   g++ -std=c++17 -O3 -DFMT_HEADER_ONLY -I$REF/include -I$REF/external/fmt/include -I$REF/external -I$REF/lib \
//       -march=x86-64-v3 -w <repo>/tools/srs_golden_gen.cpp <the sources above> -o srs_golden_gen
//   ./srs_golden_gen <repo>/tests/golden/srs_golden.npz
// It is run by no test, bench or build: the .npz it wrote is committed, and the tests read only that file.
//
// Every case: each SRS antenna port's sequence from the reference's own low-PAPR generator with the cyclic shift,
// group and mapping get_srs_information gives, one complex coefficient per (rx, tx) pair, a delay common to all
// pairs applied as a phase ramp over the absolute subcarrier index, complex Gaussian noise on every subcarrier of
// the SRS symbols, the sum rounded to bf16.  Only the grid rows of the SRS symbols are stored, by rx port INDEX
// (position in the port list), not by port number.  A case whose integer correlation peak does not stand 1.5 times
// above every sample of the search ranges more than two taps away stops the run and gets another seed (peak_margin
// below; M = 12 is held to its main-lobe ceiling of 1.31 instead).
//
// Arrays of the .npz (NN = case number, two digits):
//   names            uint8   the case names joined by '\n'
//   bandwidth        int32   [64, 4, 2] (m_SRS, N) of srs_configuration_get(c_srs, b_srs)
//   info_in          int32   [n, 10] seeded valid resources: nof_antenna_ports, configuration_index, sequence_id,
//                            bandwidth_index, comb_size, comb_offset, cyclic_shift, freq_position, freq_shift,
//                            antenna port
//   info_out         int32   [n, 7] get_srs_information of them: sequence_length, sequence_group, sequence_number,
//                            n_cs, n_cs_max, mapping_initial_subcarrier, comb_size
//   ref_estimate_us  float64 [2] single-thread time of one reference estimate() call, microseconds: 4 tx x 4 rx
//                            M = 1632 one symbol; 2 tx x 4 rx M = 144 four symbols (informative)
//   cNN_cfg          int32   [nof_antenna_ports, nof_symbols, start_symbol, configuration_index, sequence_id,
//                             bandwidth_index, comb_size, comb_offset, cyclic_shift, freq_position, freq_shift,
//                             freq_hopping, numerology, nof_rx_ports, rx_port 0..3, nof_subc]
//   cNN_x            uint16  [nof_rx_ports, nof_symbols, nof_subc, 2] cbf16 bit patterns (re, im)
//   cNN_h            float64 [nof_rx_ports, nof_antenna_ports, 2] the channel coefficients applied
//   cNN_chan         float64 [2] delay in seconds, noise standard deviation per subcarrier
//   cNN_mat          float32 [nof_rx_ports, nof_antenna_ports, 2] srs_estimator_result::channel_matrix
//   cNN_pow          float32 [epre_dB, rsrp_dB, noise_variance]
//   cNN_ta           float64 [time_alignment, resolution, min, max] seconds
#include "phy/generic_functions/dft_processor_generic_impl.h"
#include "phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "phy/upper/signal_processors/srs/srs_estimator_generic_impl.h"
#include "srsran/phy/support/resource_grid_reader.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_configuration.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_result.h"
#include "srsran/ran/srs/srs_bandwidth_configuration.h"
#include "srsran/ran/srs/srs_information.h"

#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    const char* descr = std::is_same<T, double>::value     ? "<f8"
                        : std::is_same<T, float>::value    ? "<f4"
                        : std::is_same<T, int32_t>::value  ? "<i4"
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

// ---- a resource grid the estimator can read --------------------------------------------------------------------
class grid_reader : public resource_grid_reader
{
public:
  grid_reader(unsigned ports_, unsigned subc_) : ports(ports_), subc(subc_), data(size_t(ports_) * 14 * subc_) {}
  unsigned      get_nof_ports() const override { return ports; }
  unsigned      get_nof_subc() const override { return subc; }
  unsigned      get_nof_symbols() const override { return 14; }
  bool          is_empty(unsigned) const override { return false; }
  bool          is_empty() const override { return false; }
  span<cf_t>    get(span<cf_t>, unsigned, unsigned, unsigned, const bounded_bitset<MAX_RB * NRE>&) const override { std::abort(); }
  span<cbf16_t> get(span<cbf16_t>, unsigned, unsigned, unsigned, const bounded_bitset<MAX_RB * NRE>&) const override { std::abort(); }
  void          get(span<cf_t> symbols, unsigned port, unsigned l, unsigned k_init, unsigned stride) const override
  {
    const cbf16_t* row = &data[(size_t(port) * 14 + l) * subc];
    for (size_t i = 0; i != symbols.size(); ++i) {
      if (k_init + i * stride >= subc) {
        std::abort();
      }
      symbols[i] = to_cf(row[k_init + i * stride]);
    }
  }
  void                get(span<cbf16_t>, unsigned, unsigned, unsigned) const override { std::abort(); }
  span<const cbf16_t> get_view(unsigned port, unsigned l) const override
  {
    return span<const cbf16_t>(data).subspan((size_t(port) * 14 + l) * subc, subc);
  }
  cbf16_t& at(unsigned port, unsigned l, unsigned k) { return data[(size_t(port) * 14 + l) * subc + k]; }

  unsigned             ports, subc;
  std::vector<cbf16_t> data;
};

struct test_case {
  const char*           name;
  unsigned              nof_ap, nof_symbols, start_symbol, c_srs, sequence_id, b_srs, comb, comb_offset, cyclic_shift;
  unsigned              freq_position, freq_shift, freq_hopping, numerology;
  std::vector<unsigned> rx_ports;
  double                delay_fraction; // of the measurable range max_ta_samples / sampling rate
  double                noise_sigma;    // per subcarrier; amplitude < 0: an all-zero grid
  double                amplitude;
  uint64_t              seed;
};

srs_estimator_configuration make_config(const test_case& c)
{
  srs_estimator_configuration cfg;
  cfg.slot                         = slot_point(c.numerology, 0);
  cfg.resource.nof_antenna_ports   = static_cast<srs_resource_configuration::one_two_four_enum>(c.nof_ap);
  cfg.resource.nof_symbols         = static_cast<srs_resource_configuration::one_two_four_enum>(c.nof_symbols);
  cfg.resource.start_symbol        = c.start_symbol;
  cfg.resource.configuration_index = c.c_srs;
  cfg.resource.sequence_id         = c.sequence_id;
  cfg.resource.bandwidth_index     = c.b_srs;
  cfg.resource.comb_size           = static_cast<srs_resource_configuration::comb_size_enum>(c.comb);
  cfg.resource.comb_offset         = c.comb_offset;
  cfg.resource.cyclic_shift        = c.cyclic_shift;
  cfg.resource.freq_position       = c.freq_position;
  cfg.resource.freq_shift          = c.freq_shift;
  cfg.resource.freq_hopping        = c.freq_hopping;
  cfg.resource.hopping             = srs_resource_configuration::group_or_sequence_hopping_enum::neither;
  for (unsigned p : c.rx_ports) {
    cfg.ports.push_back(p);
  }
  return cfg;
}

std::unique_ptr<srs_estimator_generic_impl> make_estimator()
{
  time_alignment_estimator_dft_impl::collection_dft_processors dfts;
  for (unsigned n = time_alignment_estimator_dft_impl::min_dft_size; n <= time_alignment_estimator_dft_impl::max_dft_size;
       n *= 2) {
    dft_processor::configuration dc{n, dft_processor::direction::INVERSE};
    dfts.emplace(n, std::make_unique<dft_processor_generic_impl>(dc));
  }
  srs_estimator_generic_impl::dependencies deps;
  deps.sequence_generator = std::make_unique<low_papr_sequence_generator_impl>();
  deps.ta_estimator       = std::make_unique<time_alignment_estimator_dft_impl>(std::move(dfts));
  return std::make_unique<srs_estimator_generic_impl>(std::move(deps), MAX_RB);
}

double gauss(std::mt19937_64& rng)
{
  // Box-Muller on the generator's raw output (the standard fixes mt19937_64, not the distributions)
  const double u1 = (double(rng() >> 11) + 1.0) / 9007199254740993.0;
  const double u2 = double(rng() >> 11) / 9007199254740992.0;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
}

unsigned idft_size_of(unsigned M)
{
  unsigned need = (M * 4096) / 3300, n = 128;
  while (n < need) {
    n *= 2;
  }
  return n;
}

// last subcarrier any antenna port of the resource uses, plus one
unsigned resource_end(const srs_estimator_configuration& cfg, unsigned nof_ap)
{
  unsigned end = 0;
  for (unsigned p = 0; p != nof_ap; ++p) {
    srs_information info = get_srs_information(cfg.resource, p);
    end = std::max(end, info.mapping_initial_subcarrier + (info.sequence_length - 1) * info.comb_size + 1);
  }
  return end;
}

struct filled {
  std::unique_ptr<grid_reader> grid;
  std::vector<double>          h;
  double                       delay_s;
  unsigned                     nof_subc;
  unsigned                     idft_size, max_ta_samples;
};

filled fill(const test_case& c, const srs_estimator_configuration& cfg)
{
  std::mt19937_64 rng(c.seed);
  filled          f;
  // an odd margin above the resource, so that rows are not a whole number of resource blocks
  f.nof_subc           = resource_end(cfg, c.nof_ap) + 5 + c.seed % 7;
  unsigned grid_ports  = 0;
  for (unsigned p : c.rx_ports) {
    grid_ports = std::max(grid_ports, p + 1);
  }
  f.grid = std::make_unique<grid_reader>(grid_ports, f.nof_subc);
  const unsigned nof_rx = c.rx_ports.size();
  srs_information info0 = get_srs_information(cfg.resource, 0);
  const unsigned  N     = idft_size_of(info0.sequence_length);
  const double    scs   = 15000.0 * (1u << c.numerology);
  const double    rate  = double(N) * scs * c.comb;
  const double    half_cp = 72.0 * 64.0 / (480000.0 * 4096.0) / double(1u << c.numerology);
  const double    max_ta  = 1.0 / (double(info0.n_cs_max) * scs * c.comb);
  const unsigned  max_ta_samples =
      std::min(unsigned(std::floor(half_cp * rate)), unsigned(std::floor(max_ta * rate)));
  f.delay_s        = c.delay_fraction * double(max_ta_samples) / rate;
  f.idft_size      = N;
  f.max_ta_samples = max_ta_samples;
  f.h.assign(size_t(nof_rx) * c.nof_ap * 2, 0.0);
  if (c.amplitude < 0) {
    return f;
  }
  low_papr_sequence_generator_impl    gen;
  std::vector<std::complex<double>>   sum(size_t(nof_rx) * f.nof_subc);
  for (unsigned r = 0; r != nof_rx; ++r) {
    for (unsigned p = 0; p != c.nof_ap; ++p) {
      const double mag = c.amplitude * (0.5 + double(rng() >> 11) / 9007199254740992.0);
      const double ph  = 2.0 * M_PI * double(rng() >> 11) / 9007199254740992.0;
      f.h[(size_t(r) * c.nof_ap + p) * 2]     = mag * std::cos(ph);
      f.h[(size_t(r) * c.nof_ap + p) * 2 + 1] = mag * std::sin(ph);
    }
  }
  for (unsigned p = 0; p != c.nof_ap; ++p) {
    srs_information   info = get_srs_information(cfg.resource, p);
    std::vector<cf_t> seq(info.sequence_length);
    gen.generate(seq, info.sequence_group, info.sequence_number, info.n_cs, info.n_cs_max);
    for (unsigned r = 0; r != nof_rx; ++r) {
      const std::complex<double> h(f.h[(size_t(r) * c.nof_ap + p) * 2], f.h[(size_t(r) * c.nof_ap + p) * 2 + 1]);
      for (unsigned n = 0; n != info.sequence_length; ++n) {
        const unsigned k = info.mapping_initial_subcarrier + n * info.comb_size;
        const double   a = -2.0 * M_PI * double(k) * scs * f.delay_s;
        sum[size_t(r) * f.nof_subc + k] += h * std::complex<double>(seq[n].real(), seq[n].imag()) * std::polar(1.0, a);
      }
    }
  }
  for (unsigned r = 0; r != nof_rx; ++r) {
    for (unsigned s = 0; s != c.nof_symbols; ++s) {
      for (unsigned k = 0; k != f.nof_subc; ++k) {
        std::complex<double> v = sum[size_t(r) * f.nof_subc + k];
        if (c.noise_sigma > 0) {
          v += std::complex<double>(gauss(rng), gauss(rng)) * (c.noise_sigma / std::sqrt(2.0));
        }
        f.grid->at(c.rx_ports[r], c.start_symbol + s, k) = cbf16_t(cf_t(float(v.real()), float(v.imag())));
      }
    }
  }
  return f;
}

// Conditioning of a case: the ratio of the integer correlation peak to the largest sample more than two taps away
// inside the two search ranges, the smallest over the antenna ports, from a direct transform in double.  A case below
// 1.5 gets another seed -- except M = 12, whose main lobe (128 / 12 taps) is wider than its search range, so that the
// ratio cannot exceed 1 / sinc^2(36 / 128) = 1.31 whatever the seed (tests/test_srs_model.py holds both).
double peak_margin(const test_case& c, const srs_estimator_configuration& cfg, const filled& f)
{
  low_papr_sequence_generator_impl gen;
  const int                        m = f.max_ta_samples, N = f.idft_size;
  double                           worst = INFINITY;
  for (unsigned p = 0; p != c.nof_ap; ++p) {
    srs_information   info = get_srs_information(cfg.resource, p);
    std::vector<cf_t> seq(info.sequence_length);
    gen.generate(seq, info.sequence_group, info.sequence_number, info.n_cs, info.n_cs_max);
    std::vector<double> corr(2 * m, 0.0); // taps -m .. m - 1
    for (unsigned r = 0; r != c.rx_ports.size(); ++r) {
      std::vector<std::complex<double>> lse(info.sequence_length);
      for (unsigned n = 0; n != info.sequence_length; ++n) {
        std::complex<double> a = 0;
        for (unsigned s = 0; s != c.nof_symbols; ++s) {
          cf_t v = to_cf(f.grid->at(c.rx_ports[r], c.start_symbol + s, info.mapping_initial_subcarrier + n * info.comb_size));
          a += std::complex<double>(v.real(), v.imag());
        }
        lse[n] = a * std::conj(std::complex<double>(seq[n].real(), seq[n].imag()));
      }
      for (int t = -m; t != m; ++t) {
        std::complex<double> x = 0;
        for (unsigned n = 0; n != info.sequence_length; ++n) {
          x += lse[n] * std::polar(1.0, 2.0 * M_PI * double((long(n) * t) % N) / N);
        }
        corr[t + m] += std::norm(x);
      }
    }
    int best_d = 0, best_a = -m;
    for (int t = 0; t != m; ++t) {
      best_d = corr[t + m] > corr[best_d + m] ? t : best_d;
      best_a = corr[t] > corr[best_a + m] ? t - m : best_a;
    }
    const int idx = corr[best_d + m] >= corr[best_a + m] ? best_d : best_a;
    double    far = 0;
    for (int t = -m; t != m; ++t) {
      if (std::abs(t - idx) > 2) {
        far = std::max(far, corr[t + m]);
      }
    }
    worst = std::min(worst, corr[idx + m] / far);
  }
  return worst;
}

double time_estimate(const test_case& c)
{
  srs_estimator_configuration cfg = make_config(c);
  filled                      f   = fill(c, cfg);
  auto                        est = make_estimator();
  volatile float              sink = 0;
  for (int i = 0; i < 3; ++i) {
    sink = sink + est->estimate(*f.grid, cfg).noise_variance.value();
  }
  const int  reps = 200;
  const auto t0   = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) {
    sink = sink + est->estimate(*f.grid, cfg).noise_variance.value();
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
  // c_srs / b_srs -> m_SRS: 0/0 4, 1/0 8, 9/0 32, 9/1 16, 12/0 48, 14/0 52, 25/1 52, 34/0 136, 61/0 272, 61/1 136
  // name, ap, symbols, start, c_srs, id, b_srs, comb, offset, cs, n_rrc, n_shift, b_hop, mu, rx, delay, sigma, amp, seed
  const std::vector<test_case> cases = {
      {"m12_comb4_1x1", 1, 1, 13, 0, 7, 0, 4, 3, 5, 0, 0, 0, 1, {0}, 0.4, 0.3, 1.0, 201},
      {"m24_comb2_2x2_2sym", 2, 2, 12, 0, 40, 0, 2, 1, 3, 0, 2, 0, 1, {0, 1}, -0.5, 0.5, 1.0, 202},
      {"m24_comb4_1x3ports_list20", 1, 2, 8, 1, 101, 0, 4, 0, 11, 0, 1, 3, 0, {2, 0}, 0.0, 0.7, 1.0, 203},
      {"m144_comb4_2x4_4sym", 2, 4, 10, 12, 5, 0, 4, 2, 1, 0, 3, 0, 1, {0, 1, 2, 3}, 0.6, 1.0, 1.0, 204},
      {"m144_comb4_4x4_cs_low", 4, 1, 9, 12, 600, 0, 4, 1, 2, 0, 0, 0, 1, {0, 1, 2, 3}, -0.3, 0.5, 1.0, 205},
      {"m144_comb4_4x2_cs_high", 4, 2, 6, 12, 77, 0, 4, 3, 7, 0, 0, 0, 0, {1, 0}, 0.5, 0.5, 1.0, 206},
      {"m96_comb2_4x4_cs_low", 4, 1, 13, 9, 1023, 1, 2, 0, 3, 5, 4, 1, 1, {3, 2, 1, 0}, 0.3, 0.4, 1.0, 207},
      {"m96_comb2_4x2_cs_high_4sym", 4, 4, 4, 9, 333, 1, 2, 1, 6, 9, 1, 2, 1, {0, 1}, -0.6, 0.6, 1.0, 208},
      {"m156_comb4_1x2", 1, 1, 11, 14, 29, 0, 4, 1, 0, 0, 7, 0, 1, {0, 1}, 0.7, 0.5, 1.0, 209},
      {"m156_comb4_bsrs1_2x1", 2, 1, 12, 25, 30, 1, 4, 2, 4, 17, 3, 1, 0, {0}, -0.2, 0.3, 1.0, 210},
      {"m408_comb4_2x2", 2, 1, 13, 34, 512, 0, 4, 0, 9, 0, 0, 0, 1, {0, 1}, 0.45, 1.0, 1.0, 211},
      {"m816_comb2_1x2_mu0", 1, 1, 10, 34, 250, 0, 2, 1, 7, 0, 5, 0, 0, {1, 0}, -0.7, 0.8, 1.0, 212},
      {"m816_comb4_4x1_cs_high", 4, 1, 12, 61, 18, 0, 4, 0, 8, 0, 0, 0, 1, {0}, 0.25, 0.5, 1.0, 213},
      {"m1632_comb2_2x2", 2, 1, 13, 61, 999, 0, 2, 0, 2, 0, 0, 0, 1, {0, 1}, 0.55, 1.0, 1.0, 214},
      {"m1632_comb2_4x1_cs_high", 4, 1, 8, 61, 64, 0, 2, 1, 5, 0, 1, 0, 1, {0}, -0.4, 0.7, 1.0, 215},
      {"m816_comb2_bsrs1_1x1_noiseless", 1, 1, 13, 61, 3, 1, 2, 0, 0, 34, 0, 3, 1, {0}, 0.35, 0.0, 1.0, 216},
      {"m48_comb2_2x2_noiseless_4sym", 2, 4, 0, 1, 11, 0, 2, 1, 1, 0, 0, 0, 0, {0, 1}, 0.0, 0.0, 1.0, 217},
      {"m48_comb2_1x2_snr0", 1, 2, 5, 1, 12, 0, 2, 0, 4, 0, 6, 0, 1, {0, 1}, 0.5, 1.0, 1.0, 218},
      {"m144_comb4_2x2_all_zero", 2, 1, 13, 12, 1, 0, 4, 0, 0, 0, 0, 0, 1, {0, 1}, 0.0, 0.0, -1.0, 219},
  };

  npz_writer  npz;
  std::string names;
  auto        est = make_estimator();
  for (size_t i = 0; i != cases.size(); ++i) {
    const test_case& c = cases[i];
    names += (i ? "\n" : "") + std::string(c.name);
    srs_estimator_configuration cfg = make_config(c);
    filled                      f   = fill(c, cfg);
    srs_estimator_result        res = est->estimate(*f.grid, cfg);
    const unsigned              nof_rx = c.rx_ports.size();
    const double                margin = c.amplitude < 0 ? INFINITY : peak_margin(c, cfg, f);
    const unsigned              M      = get_srs_information(cfg.resource, 0).sequence_length;
    if (margin < (M == 12 ? 0.9 * 1.306 : 1.5)) {
      std::fprintf(stderr, "%s: peak margin %.2f is below the cap: give the case another seed\n", c.name, margin);
      return 1;
    }

    char key[16];
    std::snprintf(key, sizeof(key), "c%02zu_", i);
    const std::string    k = key;
    std::vector<int32_t> cfgv = {int32_t(c.nof_ap),      int32_t(c.nof_symbols),  int32_t(c.start_symbol),
                                 int32_t(c.c_srs),       int32_t(c.sequence_id),  int32_t(c.b_srs),
                                 int32_t(c.comb),        int32_t(c.comb_offset),  int32_t(c.cyclic_shift),
                                 int32_t(c.freq_position), int32_t(c.freq_shift), int32_t(c.freq_hopping),
                                 int32_t(c.numerology),  int32_t(nof_rx)};
    for (unsigned r = 0; r != 4; ++r) {
      cfgv.push_back(r < nof_rx ? int32_t(c.rx_ports[r]) : 0);
    }
    cfgv.push_back(int32_t(f.nof_subc));
    npz.add<int32_t>(k + "cfg", cfgv);
    static_assert(sizeof(cbf16_t) == 4, "cbf16_t is two 16-bit halves");
    std::vector<uint16_t> x(size_t(nof_rx) * c.nof_symbols * f.nof_subc * 2);
    for (unsigned r = 0; r != nof_rx; ++r) {
      for (unsigned s = 0; s != c.nof_symbols; ++s) {
        std::memcpy(&x[(size_t(r) * c.nof_symbols + s) * f.nof_subc * 2],
                    &f.grid->at(c.rx_ports[r], c.start_symbol + s, 0),
                    size_t(f.nof_subc) * 4);
      }
    }
    npz.add<uint16_t>(k + "x", x, {nof_rx, c.nof_symbols, f.nof_subc, 2});
    npz.add<double>(k + "h", f.h, {nof_rx, c.nof_ap, 2});
    npz.add<double>(k + "chan", {f.delay_s, c.noise_sigma});
    std::vector<float> mat;
    for (unsigned r = 0; r != nof_rx; ++r) {
      for (unsigned p = 0; p != c.nof_ap; ++p) {
        const cf_t v = res.channel_matrix.get_coefficient(r, p);
        mat.push_back(v.real());
        mat.push_back(v.imag());
      }
    }
    npz.add<float>(k + "mat", mat, {nof_rx, c.nof_ap, 2});
    npz.add<float>(k + "pow", {res.epre_dB.value(), res.rsrp_dB.value(), res.noise_variance.value()});
    npz.add<double>(k + "ta", {res.time_alignment.time_alignment, res.time_alignment.resolution,
                               res.time_alignment.min, res.time_alignment.max});
    std::printf("%-34s subc %4u margin %6.2f  epre %8.3f rsrp %8.3f nv %.5g  ta %+.4e (sent %+.4e, res %.3e) min %.3e max %.3e\n",
                c.name, f.nof_subc, margin, res.epre_dB.value(), res.rsrp_dB.value(), res.noise_variance.value(),
                res.time_alignment.time_alignment, f.delay_s, res.time_alignment.resolution, res.time_alignment.min,
                res.time_alignment.max);
  }
  npz.add<uint8_t>("names", std::vector<uint8_t>(names.begin(), names.end()));

  std::vector<int32_t> bw;
  for (unsigned c_srs = 0; c_srs != 64; ++c_srs) {
    for (unsigned b_srs = 0; b_srs != 4; ++b_srs) {
      auto v = srs_configuration_get(c_srs, b_srs);
      bw.push_back(v ? int32_t(v->m_srs) : -1);
      bw.push_back(v ? int32_t(v->N) : -1);
    }
  }
  npz.add<int32_t>("bandwidth", bw, {64, 4, 2});

  std::mt19937_64      rng(4242);
  std::vector<int32_t> info_in, info_out;
  const unsigned       nof_info = 500;
  for (unsigned i = 0; i != nof_info; ++i) {
    test_case c{};
    c.nof_ap        = 1u << (rng() % 3);
    c.nof_symbols   = 1;
    c.c_srs         = rng() % 64;
    c.sequence_id   = rng() % 1024;
    c.b_srs         = rng() % 4;
    c.comb          = (rng() & 1) ? 4 : 2;
    c.comb_offset   = rng() % c.comb;
    c.cyclic_shift  = rng() % (c.comb == 4 ? 12 : 8);
    c.freq_position = rng() % 68;
    c.freq_shift    = rng() % 269;
    c.freq_hopping  = c.b_srs + rng() % (4 - c.b_srs);
    c.rx_ports      = {0};
    const unsigned              ap  = rng() % c.nof_ap;
    srs_estimator_configuration cfg = make_config(c);
    srs_information             info = get_srs_information(cfg.resource, ap);
    info_in.insert(info_in.end(), {int32_t(c.nof_ap), int32_t(c.c_srs), int32_t(c.sequence_id), int32_t(c.b_srs),
                                   int32_t(c.comb), int32_t(c.comb_offset), int32_t(c.cyclic_shift),
                                   int32_t(c.freq_position), int32_t(c.freq_shift), int32_t(ap)});
    info_out.insert(info_out.end(), {int32_t(info.sequence_length), int32_t(info.sequence_group),
                                     int32_t(info.sequence_number), int32_t(info.n_cs), int32_t(info.n_cs_max),
                                     int32_t(info.mapping_initial_subcarrier), int32_t(info.comb_size)});
  }
  npz.add<int32_t>("info_in", info_in, {nof_info, 10});
  npz.add<int32_t>("info_out", info_out, {nof_info, 7});

  const test_case t0 = {"time_4x4_m1632", 4, 1, 13, 61, 1, 0, 2, 0, 0, 0, 0, 0, 1, {0, 1, 2, 3}, 0.3, 1.0, 1.0, 1};
  const test_case t1 = {"time_2x4_m144", 2, 4, 10, 12, 1, 0, 4, 0, 0, 0, 0, 0, 1, {0, 1, 2, 3}, 0.3, 1.0, 1.0, 2};
  const double    us0 = time_estimate(t0), us1 = time_estimate(t1);
  std::printf("reference estimate(), one thread: 4x4 M=1632 1 symbol %.1f us, 2x4 M=144 4 symbols %.1f us\n", us0, us1);
  npz.add<double>("ref_estimate_us", {us0, us1});
  if (!npz.save(argv[1])) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  return 0;
}
