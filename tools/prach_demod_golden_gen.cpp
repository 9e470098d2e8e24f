// prach_demod_golden_gen.cpp -- writes tests/golden/prach_demod_golden.npz: seeded PRACH windows and what the
// reference's OFDM PRACH demodulator (ofdm_prach_demodulator_impl over dft_processor_generic_impl) makes of them.
//
// NEEDS THE REFERENCE TREE (srsRAN Project): it is compiled together with the reference's own sources
//   lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp, lib/phy/generic_functions/dft_processor_generic_impl.cpp,
//   lib/ran/prach/prach_preamble_information.cpp, lib/ran/prach/prach_frequency_mapping.cpp and lib/srsvec/*.cpp
// with the flags of oracle/Makefile (CXXFLAGS_REF), e.g. from a directory outside this repository:
//   g++ -std=c++17 -O3 -DFMT_HEADER_ONLY -I$REF/include -I$REF/external/fmt/include -I$REF/external -I$REF/lib \
//       -march=x86-64-v3 -w <repo>/tools/prach_demod_golden_gen.cpp <the sources above> -o prach_demod_golden_gen
//   ./prach_demod_golden_gen <repo>/tests/golden/prach_demod_golden.npz
// It is run by no test, bench or build: the .npz it wrote is committed, and the tests read only that file.
//
// The input samples are NOT stored.  Every fixture records a seed; the samples are the bytes of a splitmix64 stream
// (tests/prach_demod_model.py holds the same generator): word j = splitmix64(seed + (j + 1) 0x9E3779B97F4A7C15), its
// bytes from the least significant, sample n = ((byte 2n) - 128) / 128 + i ((byte 2n + 1) - 128) / 128, over the whole
// buffer of nof_ports x port_stride samples.  checksum = sum over the bytes of byte_i x (i mod 65521 + 1) mod 2^63.
// A `boost` fixture multiplies every sample outside the DFT windows (cyclic prefixes, gaps, tail, port padding) by 64.
// A seed is kept only when the share of the reference's bf16 words that differ from the exactly computed bins
// (double-precision direct sums, scaled in double, rounded once, half to even) is at most 1e-3; else seed + 1 is tried.
//
// Where the reference would assert (or read out of bounds with assertions compiled out) the tool checks first and
// records the fixture as rejected, with no geometry and no output.
//
// Arrays of the .npz (NN = fixture number, two digits):
//   names     uint8  the fixture names joined by '\n'
//   fNN_cfg   int32  [srate_hz, numerology, subframe_slot_index, format, nof_td_occasions, nof_fd_occasions,
//                     start_symbol, rb_offset, nof_prb_ul_grid, nof_ports, port_stride, nof_samples, boost, rejected]
//                    format: 0..3, then A1 A2 A3 B1 B4 C0 C2 A1/B1 A2/B2 A3/B3 = 4..13
//   fNN_seed  int64  [seed, checksum]
//   fNN_geo   int32  [ra_scs, L_ra, dft_size, nof_symbols, window_samples]  (ra_scs: 0 = 15, 1 = 30, 2 = 60, 3 = 120,
//                     4 = 1.25, 5 = 5 kHz; window_samples from get_prach_window_duration)
//   fNN_td    int32  [nof_td, 2] (sample_offset, cp_samples) per time-domain occasion
//   fNN_k     int32  [nof_fd] k_start per frequency-domain occasion
//   fNN_out   uint16 [nof_td, nof_fd, nof_ports, nof_symbols, L_ra, 2] cbf16 bit patterns (re, im)
//   fNN_share float64 [1] share of the reference's words that differ from the exact bins (<= 1e-3)
#include "phy/generic_functions/dft_processor_generic_impl.h"
#include "phy/lower/modulation/ofdm_prach_demodulator_impl.h"
#include "srsran/phy/constants.h"
#include "srsran/phy/support/prach_buffer.h"
#include "srsran/ran/prach/prach_constants.h"
#include "srsran/ran/prach/prach_frequency_mapping.h"
#include "srsran/ran/prach/prach_preamble_information.h"

#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
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
                        : std::is_same<T, int64_t>::value  ? "<i8"
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

// ---- the PRACH buffer of one window, in the product's layout [td][fd][port][symbol][L] -------------------------
class window_buffer : public prach_buffer
{
public:
  window_buffer(unsigned td_, unsigned fd_, unsigned ports_, unsigned symbols_, unsigned L_) :
    td(td_), fd(fd_), ports(ports_), symbols(symbols_), L(L_), data(size_t(td_) * fd_ * ports_ * symbols_ * L_)
  {
  }
  unsigned get_max_nof_ports() const override { return ports; }
  unsigned get_max_nof_td_occasions() const override { return td; }
  unsigned get_max_nof_fd_occasions() const override { return fd; }
  unsigned get_max_nof_symbols() const override { return symbols; }
  unsigned get_sequence_length() const override { return L; }
  size_t   at(unsigned p, unsigned t, unsigned f, unsigned s) const
  {
    return (((size_t(t) * fd + f) * ports + p) * symbols + s) * L;
  }
  span<cbf16_t> get_symbol(unsigned p, unsigned t, unsigned f, unsigned s) override
  {
    return span<cbf16_t>(data).subspan(at(p, t, f, s), L);
  }
  span<const cbf16_t> get_symbol(unsigned p, unsigned t, unsigned f, unsigned s) const override
  {
    return span<const cbf16_t>(data).subspan(at(p, t, f, s), L);
  }
  unsigned             td, fd, ports, symbols, L;
  std::vector<cbf16_t> data;
};

struct fixture {
  const char* name;
  unsigned    srate_hz, numerology, slot_index;
  int         format; // prach_format_type value
  unsigned    nof_td, nof_fd, start_symbol, rb_offset, nof_prb, nof_ports, stride_extra;
  bool        boost;
};

constexpr int F0 = 0, F1 = 1, F2 = 2, F3 = 3, A1 = 4, A2 = 5, B4 = 8, C0 = 9, C2 = 10, A1B1 = 11, A3B3 = 13;

const fixture FIXTURES[] = {
    // long formats
    {"f0_7.68_rb0_2fd_2ports", 7680000, 0, 0, F0, 1, 2, 0, 0, 25, 2, 37, false},
    {"f0_7.68_straddle_2fd_2ports", 7680000, 0, 0, F0, 1, 2, 0, 8, 25, 2, 37, false},
    {"f0_30.72_mu1_2fd_straddle", 30720000, 1, 0, F0, 1, 2, 0, 23, 51, 1, 0, false},
    {"f0_23.04", 23040000, 0, 0, F0, 1, 1, 0, 10, 79, 1, 0, false},
    {"f3_23.04", 23040000, 0, 0, F3, 1, 1, 0, 4, 79, 1, 0, false},
    {"f1_15.36", 15360000, 0, 0, F1, 1, 1, 0, 3, 52, 1, 0, false},
    {"f2_15.36", 15360000, 0, 0, F2, 1, 1, 0, 30, 52, 1, 0, false},
    {"f3_30.72_boost", 30720000, 0, 0, F3, 1, 1, 0, 40, 106, 1, 0, true},
    {"f0_61.44_mu1", 61440000, 1, 0, F0, 1, 1, 0, 50, 106, 1, 0, false},
    {"f0_122.88_mu1_top", 122880000, 1, 0, F0, 1, 1, 0, 270, 273, 1, 0, false},
    {"f0_7.68_start2", 7680000, 0, 0, F0, 1, 1, 2, 5, 25, 1, 0, false},
    {"f0_30.72_mu1_slot1", 30720000, 1, 1, F0, 1, 1, 0, 7, 51, 1, 0, false},
    // short formats
    {"a1_30.72_mu1_6td", 30720000, 1, 0, A1, 6, 1, 0, 4, 51, 1, 0, false},
    {"a1_30.72_mu1_6td_slot1", 30720000, 1, 1, A1, 6, 1, 0, 4, 51, 1, 0, false},
    {"a1_15.36_mu0_start7_boost", 15360000, 0, 0, A1, 3, 1, 7, 20, 52, 1, 0, true},
    {"b4_30.72_mu1", 30720000, 1, 0, B4, 1, 1, 0, 0, 51, 1, 0, false},
    {"c0_30.72_mu1", 30720000, 1, 0, C0, 1, 1, 0, 30, 51, 1, 0, false},
    {"c2_30.72_mu1_start2", 30720000, 1, 0, C2, 1, 1, 2, 12, 51, 1, 0, false},
    {"a2_30.72_mu1", 30720000, 1, 0, A2, 1, 1, 0, 26, 51, 1, 0, false},
    {"a1b1_30.72_mu1_3td_start2", 30720000, 1, 0, A1B1, 3, 1, 2, 9, 51, 1, 0, false},
    {"a3b3_30.72_mu1_2td", 30720000, 1, 1, A3B3, 2, 1, 0, 17, 51, 1, 0, false},
    {"a1_30.72_mu2_2fd", 30720000, 2, 2, A1, 2, 2, 4, 0, 24, 1, 0, false},
    {"a1_122.88_mu3_4fd", 122880000, 3, 5, A1, 1, 4, 0, 12, 66, 1, 0, false},
    // what the reference asserts on
    {"rejected_k_start_past_grid", 7680000, 0, 0, F0, 1, 1, 0, 20, 25, 1, 0, false},
    {"rejected_dft_not_above_grid", 7680000, 0, 0, F0, 1, 1, 0, 0, 52, 1, 0, false},
    {"rejected_reserved_spacing_pair", 122880000, 3, 0, F0, 1, 1, 0, 0, 66, 1, 0, false},
    {"rejected_long_two_td", 7680000, 0, 0, F0, 2, 1, 0, 0, 25, 1, 0, false},
    {"rejected_short_zero_td", 30720000, 1, 0, A1, 0, 1, 0, 0, 51, 1, 0, false},
    {"rejected_nine_fd", 245760000, 3, 0, A1, 1, 9, 0, 0, 110, 1, 0, false},
};

uint64_t splitmix64(uint64_t x)
{
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// nof complex samples from the seed, and their checksum
std::vector<cf_t> generate(uint64_t seed, size_t nof, int64_t& checksum)
{
  std::vector<cf_t> x(nof);
  uint64_t          sum = 0;
  for (size_t j = 0; 4 * j < nof; ++j) {
    const uint64_t w = splitmix64(seed + (j + 1) * 0x9E3779B97F4A7C15ull);
    for (unsigned b = 0; b != 8; ++b) {
      const size_t   i    = 8 * j + b;
      const unsigned byte = (w >> (8 * b)) & 0xFF;
      if (i / 2 >= nof) {
        break;
      }
      sum += byte * (i % 65521 + 1);
      const float v = (static_cast<float>(byte) - 128.0f) / 128.0f;
      if (i & 1) {
        x[i / 2] = cf_t(x[i / 2].real(), v);
      } else {
        x[i / 2] = cf_t(v, 0.0f);
      }
    }
  }
  checksum = static_cast<int64_t>(sum & 0x7FFFFFFFFFFFFFFFull);
  return x;
}

uint16_t bf16_round(double v)
{
  // one rounding, half to even: through float, whose own rounding matters only when it lands on a bf16 tie
  const float f = static_cast<float>(v);
  uint32_t    u;
  std::memcpy(&u, &f, 4);
  if ((u & 0xFFFFu) == 0x8000u && static_cast<double>(f) != v) {
    return (u >> 16) + (std::fabs(v) > std::fabs(static_cast<double>(f)) ? 1u : 0u);
  }
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

struct geometry {
  unsigned              ra_scs, L, N, nof_symbols, window;
  std::vector<unsigned> offset, cp, k_start;
};

// The timing of ofdm_prach_demodulator_impl::demodulate, with the reference's own types and helpers; false where the
// reference would assert.
bool reference_geometry(const fixture& fx, geometry& g)
{
  const prach_format_type format = static_cast<prach_format_type>(fx.format);
  const bool              is_long = is_long_preamble(format);
  if (fx.numerology > 3) {
    return false;
  }
  const subcarrier_spacing pusch_scs = to_subcarrier_spacing(fx.numerology);
  if ((is_long && fx.nof_td != 1) || fx.nof_td == 0 || fx.nof_td > prach_constants::MAX_NOF_PRACH_TD_OCCASIONS ||
      fx.nof_fd > prach_constants::MAX_NOF_PRACH_FD_OCCASIONS) {
    return false;
  }
  static constexpr phy_time_unit sixteen_kappa = phy_time_unit::from_units_of_kappa(16);
  const phy_time_unit symbol = phy_time_unit::from_units_of_kappa((144U + 2048U) >> fx.numerology);
  for (unsigned i = 0; i != fx.nof_td; ++i) {
    prach_preamble_information info =
        is_long ? get_prach_preamble_long_info(format)
                : get_prach_preamble_short_info(format, to_ra_subcarrier_spacing(pusch_scs), i + 1 == fx.nof_td);
    phy_time_unit t_occ   = symbol * (fx.start_symbol + get_preamble_duration(format) * i);
    phy_time_unit t_slot  = symbol * fx.slot_index * 14;
    phy_time_unit t_start = t_occ + t_slot;
    if (info.scs == prach_subcarrier_spacing::kHz1_25 || info.scs == prach_subcarrier_spacing::kHz5 ||
        info.scs == prach_subcarrier_spacing::kHz15 || info.scs == prach_subcarrier_spacing::kHz30) {
      if (t_occ > phy_time_unit::from_seconds(0.0)) {
        t_occ += sixteen_kappa;
      }
      if (t_occ > phy_time_unit::from_seconds(0.5e-3)) {
        t_occ += sixteen_kappa;
      }
    }
    phy_time_unit t_end = t_start + info.cp_length + info.symbol_length();
    if (is_short_preamble(info.scs)) {
      if (t_start <= phy_time_unit::from_seconds(0.0) && t_end >= phy_time_unit::from_seconds(0.0)) {
        info.cp_length += sixteen_kappa;
      }
      if (t_start <= phy_time_unit::from_seconds(0.5e-3) && t_end >= phy_time_unit::from_seconds(0.5e-3)) {
        info.cp_length += sixteen_kappa;
      }
    }
    if (!t_occ.is_sample_accurate(fx.srate_hz) || !info.cp_length.is_sample_accurate(fx.srate_hz)) {
      return false;
    }
    const prach_frequency_mapping_information map = prach_frequency_mapping_get(info.scs, pusch_scs);
    if (map.nof_rb_ra == PRACH_FREQUENCY_MAPPING_INFORMATION_RESERVED.nof_rb_ra) {
      return false;
    }
    g.ra_scs      = static_cast<unsigned>(info.scs);
    g.L           = info.sequence_length;
    g.N           = fx.srate_hz / ra_scs_to_Hz(info.scs);
    g.nof_symbols = info.nof_symbols;
    g.offset.push_back(t_occ.to_samples(fx.srate_hz));
    g.cp.push_back(info.cp_length.to_samples(fx.srate_hz));
    const unsigned K    = scs_to_khz(pusch_scs) * 1000 / ra_scs_to_Hz(info.scs);
    const unsigned grid = fx.nof_prb * K * NRE;
    if (g.N <= grid) {
      return false;
    }
    if (i == 0) {
      for (unsigned f = 0; f != fx.nof_fd; ++f) {
        const unsigned k_start = K * NRE * (fx.rb_offset + map.nof_rb_ra * f) + map.k_bar;
        if (k_start + info.sequence_length >= grid) {
          return false;
        }
        g.k_start.push_back(k_start);
      }
    }
  }
  g.window = get_prach_window_duration(format, pusch_scs, fx.start_symbol, fx.nof_td).to_samples(fx.srate_hz);
  return true;
}

// exact bins of one symbol: DFT bin of grid subcarrier k_start + b, b < L, scaled by 1 / sqrt(N), in double
void exact_symbol(const cf_t* x, unsigned N, unsigned grid, unsigned k_start, unsigned L, std::vector<uint16_t>& words)
{
  static std::vector<double> c, s;
  static unsigned            table_n = 0;
  if (table_n != N) {
    c.resize(N), s.resize(N);
    for (unsigned m = 0; m != N; ++m) {
      const double a = -2.0 * M_PI * static_cast<double>(m) / static_cast<double>(N);
      c[m] = std::cos(a), s[m] = std::sin(a);
    }
    table_n = N;
  }
  const double scale = 1.0 / std::sqrt(static_cast<double>(N));
  for (unsigned b = 0; b != L; ++b) {
    const unsigned g   = k_start + b;
    const unsigned bin = g < grid / 2 ? N - grid / 2 + g : g - grid / 2;
    double         re = 0.0, im = 0.0;
    unsigned       t  = 0;
    for (unsigned n = 0; n != N; ++n) {
      const double xr = x[n].real(), xi = x[n].imag();
      re += xr * c[t] - xi * s[t];
      im += xr * s[t] + xi * c[t];
      t += bin;
      t = t >= N ? t - N : t;
    }
    words.push_back(bf16_round(re * scale));
    words.push_back(bf16_round(im * scale));
  }
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <output .npz>\n", argv[0]);
    return 1;
  }
  npz_writer  npz;
  std::string names;
  unsigned    index = 0;
  for (const fixture& fx : FIXTURES) {
    char key[16];
    std::snprintf(key, sizeof(key), "f%02u_", index++);
    names += std::string(names.empty() ? "" : "\n") + fx.name;
    geometry   g;
    const bool ok = reference_geometry(fx, g);
    unsigned   nof_samples = 0, stride = 0;
    if (ok) {
      unsigned need = 0;
      for (unsigned i = 0; i != fx.nof_td; ++i) {
        need = std::max(need, g.offset[i] + g.cp[i] + g.nof_symbols * g.N);
      }
      nof_samples = std::max(g.window, need);
      stride      = nof_samples + fx.stride_extra;
    }
    std::vector<int32_t> cfg = {int32_t(fx.srate_hz), int32_t(fx.numerology), int32_t(fx.slot_index), fx.format,
                                int32_t(fx.nof_td), int32_t(fx.nof_fd), int32_t(fx.start_symbol), int32_t(fx.rb_offset),
                                int32_t(fx.nof_prb), int32_t(fx.nof_ports), int32_t(stride), int32_t(nof_samples),
                                fx.boost, !ok};
    npz.add(std::string(key) + "cfg", cfg);
    if (!ok) {
      std::printf("%-34s rejected\n", fx.name);
      continue;
    }
    const subcarrier_spacing pusch_scs = to_subcarrier_spacing(fx.numerology);
    const unsigned K    = scs_to_khz(pusch_scs) * 1000 / ra_scs_to_Hz(static_cast<prach_subcarrier_spacing>(g.ra_scs));
    const unsigned grid = fx.nof_prb * K * NRE;

    ofdm_prach_demodulator_impl::dft_processors_table dfts;
    dfts.emplace(static_cast<prach_subcarrier_spacing>(g.ra_scs),
                 std::make_unique<dft_processor_generic_impl>(
                     dft_processor::configuration{g.N, dft_processor::direction::DIRECT}));
    ofdm_prach_demodulator_impl demod(sampling_rate::from_Hz(fx.srate_hz), std::move(dfts));

    for (uint64_t seed = 1000 + 17 * index;; ++seed) {
      int64_t           checksum = 0;
      std::vector<cf_t> x        = generate(seed, size_t(fx.nof_ports) * stride, checksum);
      if (fx.boost) {
        std::vector<uint8_t> inside(x.size(), 0);
        for (unsigned p = 0; p != fx.nof_ports; ++p) {
          for (unsigned i = 0; i != fx.nof_td; ++i) {
            const size_t first = size_t(p) * stride + g.offset[i] + g.cp[i];
            std::fill(inside.begin() + first, inside.begin() + first + size_t(g.nof_symbols) * g.N, 1);
          }
        }
        for (size_t n = 0; n != x.size(); ++n) {
          if (!inside[n]) {
            x[n] *= 64.0f;
          }
        }
      }
      window_buffer buffer(fx.nof_td, fx.nof_fd, fx.nof_ports, g.nof_symbols, g.L);
      for (unsigned p = 0; p != fx.nof_ports; ++p) {
        ofdm_prach_demodulator::configuration config;
        config.slot             = slot_point(fx.numerology, fx.slot_index);
        config.format           = static_cast<prach_format_type>(fx.format);
        config.nof_td_occasions = fx.nof_td;
        config.nof_fd_occasions = fx.nof_fd;
        config.start_symbol     = fx.start_symbol;
        config.rb_offset        = fx.rb_offset;
        config.nof_prb_ul_grid  = fx.nof_prb;
        config.port             = p;
        demod.demodulate(buffer, span<const cf_t>(x).subspan(size_t(p) * stride, nof_samples), config);
      }
      std::vector<uint16_t> ref, exact;
      for (const cbf16_t& v : buffer.data) {
        uint16_t re, im;
        std::memcpy(&re, &v.real, 2);
        std::memcpy(&im, &v.imag, 2);
        ref.push_back(re), ref.push_back(im);
      }
      for (unsigned t = 0; t != fx.nof_td; ++t) {
        for (unsigned f = 0; f != fx.nof_fd; ++f) {
          for (unsigned p = 0; p != fx.nof_ports; ++p) {
            for (unsigned s = 0; s != g.nof_symbols; ++s) {
              exact_symbol(x.data() + size_t(p) * stride + g.offset[t] + g.cp[t] + size_t(s) * g.N, g.N, grid,
                           g.k_start[f], g.L, exact);
            }
          }
        }
      }
      size_t differ = 0;
      for (size_t i = 0; i != ref.size(); ++i) {
        differ += ref[i] != exact[i];
      }
      const double share = static_cast<double>(differ) / static_cast<double>(ref.size());
      if (share > 1e-3) {
        std::printf("%-34s seed %llu: share %.2e, next seed\n", fx.name, (unsigned long long)seed, share);
        continue;
      }
      std::printf("%-34s N %6u seed %llu share %.2e words %zu\n", fx.name, g.N, (unsigned long long)seed, share,
                  ref.size());
      npz.add(std::string(key) + "seed", std::vector<int64_t>{int64_t(seed), checksum});
      npz.add(std::string(key) + "geo", std::vector<int32_t>{int32_t(g.ra_scs), int32_t(g.L), int32_t(g.N),
                                                             int32_t(g.nof_symbols), int32_t(g.window)});
      std::vector<int32_t> td;
      for (unsigned i = 0; i != fx.nof_td; ++i) {
        td.push_back(g.offset[i]), td.push_back(g.cp[i]);
      }
      npz.add(std::string(key) + "td", td, {fx.nof_td, 2});
      npz.add(std::string(key) + "k", std::vector<int32_t>(g.k_start.begin(), g.k_start.end()));
      npz.add(std::string(key) + "out", ref, {fx.nof_td, fx.nof_fd, fx.nof_ports, g.nof_symbols, g.L, 2});
      npz.add(std::string(key) + "share", std::vector<double>{share});
      break;
    }
  }
  npz.add("names", std::vector<uint8_t>(names.begin(), names.end()));
  if (!npz.save(argv[1])) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  std::printf("wrote %s (%zu bytes)\n", argv[1], npz.out.size());
  return 0;
}
