// csi_rs_golden_gen.cpp -- writes tests/golden/csi_rs_golden.npz: NZP-CSI-RS configurations and the grids the
// reference's generator writes for them.
//
// NEEDS THE REFERENCE TREE (srsRAN Project): it is compiled together with the reference's own sources
//   lib/phy/upper/signal_processors/nzp_csi_rs/nzp_csi_rs_generator_impl.cpp, lib/ran/csi_rs/csi_rs_pattern.cpp,
//   lib/ran/csi_rs/csi_rs_config_helpers.cpp, lib/phy/upper/sequence_generators/pseudo_random_generator_impl.cpp,
//   lib/phy/support/resource_grid_mapper_impl.cpp, resource_grid_writer_impl.cpp, re_pattern.cpp,
//   lib/phy/generic_functions/precoding/precoding_factories.cpp, channel_precoder_impl.cpp,
//   channel_precoder_generic.cpp, channel_precoder_avx2.cpp, channel_precoder_avx512.cpp (this one with AVX512FLAGS),
//   lib/srsvec/*.cpp
// with the flags of oracle/Makefile (CXXFLAGS_REF), e.g. from a directory outside this repository:
//   F="-std=c++17 -O3 -DFMT_HEADER_ONLY -I$REF/include -I$REF/external/fmt/include -I$REF/external -I$REF/lib \
//      -march=x86-64-v3 -w"
//   g++ $F -mavx512f -mavx512bw -mavx512vl -mavx512dq -mavx512cd -mavx512vbmi -c \
//       $REF/lib/phy/generic_functions/precoding/channel_precoder_avx512.cpp -o avx512.o
//   g++ $F <repo>/tools/csi_rs_golden_gen.cpp <the other sources above> avx512.o -o csi_rs_golden_gen
//   ./csi_rs_golden_gen <repo>/tests/golden/csi_rs_golden.npz
// It is run by no test, bench or build: the .npz it wrote is committed, and the tests read only that file.
//
// Every case maps its resources, in order, with sequential map() calls into one zeroed grid, once with the precoder
// create_channel_precoder_factory("auto") gives on the recording machine and once with "generic".  The "auto" grid is
// stored (only the OFDM symbol rows a resource touches); the REs where "generic" wrote other bits are listed.
// Seeded weights come from the raw output of std::mt19937_64 (the standard fixes the generator, not the
// distributions): re, im uniform in [-1, 1), rounded to float.
//
// Arrays of the .npz (NN = case number, two digits):
//   names        uint8   the case names joined by '\n'
//   precoders    uint8   what "auto" resolved to on the recording machine ("avx512", "avx2" or "generic")
//   pattern_in   int32   [300, 14] seeded valid configurations over rows 1-12: start_rb, nof_rb, row, nof_k_ref,
//                        k_ref 0..5, symbol_l0, symbol_l1, cdm, freq_density
//   pattern_out  int32   [300, 36] get_csi_rs_pattern of them: rb_begin, rb_end, rb_stride, nof_ports, then
//                        (re_mask, symbol_mask) of ports 0..15 (zero beyond nof_ports)
//   ref_map_us   float64 [2] single-thread time of one reference map() call, microseconds: row 1 and row 4 (identity
//                        weights) on 273 PRB (informative)
//   cNN_cfg      int32   [nof_resources, 19] numerology, slot_index, start_rb, nof_rb, row, nof_k_ref, k_ref 0..5,
//                        symbol_l0, symbol_l1, cdm, freq_density, scrambling_id, nof_grid_ports, nof_subc
//                        (cdm: 0 none, 1 fd-CDM2, 2 cdm4-FD2-TD2, 3 cdm8-FD2-TD4; freq_density: 0 three, 1 one,
//                         2 dot5 even RB, 3 dot5 odd RB -- the codes of include/srsran_amd/csi_rs.h)
//   cNN_amp      float32 [nof_resources] amplitude
//   cNN_w        float32 [nof_resources, 4, 4, 2] precoding weights [CSI-RS port][tx port][re, im] (zero beyond the row)
//   cNN_symbols  int32   [nof_rows] the OFDM symbols stored
//   cNN_grid     uint16  [nof_grid_ports, nof_rows, nof_subc, 2] cbf16 bit patterns (re, im), "auto" precoder
//   cNN_gen_idx  int32   [m] flat indices into [nof_grid_ports, nof_rows, nof_subc] where "generic" differs
//   cNN_gen_val  uint16  [m, 2] the "generic" bit patterns there
#include "phy/support/resource_grid_mapper_impl.h"
#include "phy/support/resource_grid_writer_impl.h"
#include "phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "phy/upper/signal_processors/nzp_csi_rs/nzp_csi_rs_generator_impl.h"
#include "srsran/phy/generic_functions/precoding/precoding_factories.h"
#include "srsran/ran/csi_rs/csi_rs_pattern.h"
#include "srsran/support/cpu_features.h"

#include <atomic>
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

// ---- configurations --------------------------------------------------------------------------------------------
enum { CDM_NONE = 0, CDM_FD2 = 1, CDM_FD2_TD2 = 2, CDM_FD2_TD4 = 3 };
enum { D_THREE = 0, D_ONE = 1, D_EVEN = 2, D_ODD = 3 };

csi_rs_cdm_type to_cdm(unsigned v)
{
  return static_cast<csi_rs_cdm_type>(v); // the same order: no_CDM, fd_CDM2, cdm4_FD2_TD2, cdm8_FD2_TD4
}

csi_rs_freq_density_type to_density(unsigned v)
{
  switch (v) {
    case D_THREE:
      return csi_rs_freq_density_type::three;
    case D_ONE:
      return csi_rs_freq_density_type::one;
    case D_EVEN:
      return csi_rs_freq_density_type::dot5_even_RB;
    default:
      return csi_rs_freq_density_type::dot5_odd_RB;
  }
}

enum weight_kind { W_IDENTITY, W_SCALAR, W_SEEDED, W_PERMUTATION };

struct resource {
  unsigned              numerology, slot_index, start_rb, nof_rb, row;
  std::vector<unsigned> k_ref;
  unsigned              l0, cdm, density, scrambling_id;
  float                 amplitude;
  weight_kind           wk;
  std::complex<float>   scalar; // W_SCALAR: the one-port weight; W_PERMUTATION: the scale
  uint64_t              seed;
};

struct test_case {
  const char*           name;
  unsigned              nof_grid_ports, nof_subc;
  std::vector<resource> resources;
};

unsigned ports_of_row(unsigned row)
{
  static const unsigned n[13] = {0, 1, 1, 2, 4, 4, 8, 8, 8, 12, 12, 16, 16};
  return n[row];
}

// [CSI-RS port][tx port]
std::vector<std::complex<float>> weights_of(const resource& r)
{
  const unsigned                   n = ports_of_row(r.row);
  std::vector<std::complex<float>> w(16, 0.0F);
  std::mt19937_64                  rng(r.seed);
  for (unsigned i = 0; i != n; ++i) {
    for (unsigned p = 0; p != n; ++p) {
      switch (r.wk) {
        case W_IDENTITY:
          w[4 * i + p] = i == p ? 1.0F : 0.0F;
          break;
        case W_SCALAR:
          w[4 * i + p] = r.scalar;
          break;
        case W_PERMUTATION: // CSI-RS port i on tx port (i + 1) mod n
          w[4 * i + p] = p == (i + 1) % n ? r.scalar : 0.0F;
          break;
        case W_SEEDED: {
          const double re = double(rng() >> 11) / 4503599627370496.0 - 1.0;
          const double im = double(rng() >> 11) / 4503599627370496.0 - 1.0;
          w[4 * i + p]    = std::complex<float>(float(re), float(im));
          break;
        }
      }
    }
  }
  return w;
}

nzp_csi_rs_generator::config_t make_config(const resource& r)
{
  nzp_csi_rs_generator::config_t cfg;
  cfg.slot                     = slot_point(r.numerology, r.slot_index);
  cfg.cp                       = cyclic_prefix::NORMAL;
  cfg.start_rb                 = r.start_rb;
  cfg.nof_rb                   = r.nof_rb;
  cfg.csi_rs_mapping_table_row = r.row;
  for (unsigned k : r.k_ref) {
    cfg.freq_allocation_ref_idx.push_back(k);
  }
  cfg.symbol_l0     = r.l0;
  cfg.symbol_l1     = 0;
  cfg.cdm           = to_cdm(r.cdm);
  cfg.freq_density  = to_density(r.density);
  cfg.scrambling_id = r.scrambling_id;
  cfg.amplitude     = r.amplitude;
  const unsigned n  = ports_of_row(r.row);
  cfg.precoding     = precoding_configuration(n, n, 1, MAX_RB);
  const auto w      = weights_of(r);
  for (unsigned i = 0; i != n; ++i) {
    for (unsigned p = 0; p != n; ++p) {
      cfg.precoding.set_coefficient(w[4 * i + p], i, p, 0);
    }
  }
  return cfg;
}

csi_rs_pattern pattern_of(const resource& r)
{
  csi_rs_pattern_configuration pc;
  pc.start_rb                 = r.start_rb;
  pc.nof_rb                   = r.nof_rb;
  pc.csi_rs_mapping_table_row = r.row;
  for (unsigned k : r.k_ref) {
    pc.freq_allocation_ref_idx.push_back(k);
  }
  pc.symbol_l0    = r.l0;
  pc.symbol_l1    = 0;
  pc.cdm          = to_cdm(r.cdm);
  pc.freq_density = to_density(r.density);
  return get_csi_rs_pattern(pc);
}

template <size_t N>
int32_t mask_of(const bounded_bitset<N>& b)
{
  int32_t m = 0;
  for (size_t i = 0; i != b.size(); ++i) {
    m |= b.test(i) ? (1 << i) : 0;
  }
  return m;
}

using grid_tensor = dynamic_tensor<static_cast<unsigned>(resource_grid_dimensions::all), cbf16_t, resource_grid_dimensions>;

std::unique_ptr<nzp_csi_rs_generator_impl> make_generator(const char* precoder)
{
  std::unique_ptr<channel_precoder> p = create_channel_precoder_factory(precoder)->create();
  if (!p) {
    std::fprintf(stderr, "no %s precoder\n", precoder);
    std::exit(1);
  }
  return std::make_unique<nzp_csi_rs_generator_impl>(std::make_unique<pseudo_random_generator_impl>(),
                                                     std::make_unique<resource_grid_mapper_impl>(std::move(p)));
}

// The case's resources mapped in order into a zeroed grid; returns [port][14][subc] as (re, im) bit patterns.
std::vector<uint16_t> run_case(const test_case& c, nzp_csi_rs_generator& gen)
{
  grid_tensor           data({c.nof_subc, MAX_NSYMB_PER_SLOT, c.nof_grid_ports});
  std::atomic<unsigned> empty{0};
  for (unsigned p = 0; p != c.nof_grid_ports; ++p) {
    for (unsigned l = 0; l != MAX_NSYMB_PER_SLOT; ++l) {
      span<cbf16_t> row = data.get_view<static_cast<unsigned>(resource_grid_dimensions::symbol)>({l, p});
      std::memset(row.data(), 0, row.size() * sizeof(cbf16_t));
    }
  }
  resource_grid_writer_impl writer(data, empty);
  for (const resource& r : c.resources) {
    gen.map(writer, make_config(r));
  }
  static_assert(sizeof(cbf16_t) == 4, "cbf16_t is two 16-bit halves");
  std::vector<uint16_t> out(size_t(c.nof_grid_ports) * MAX_NSYMB_PER_SLOT * c.nof_subc * 2);
  for (unsigned p = 0; p != c.nof_grid_ports; ++p) {
    for (unsigned l = 0; l != MAX_NSYMB_PER_SLOT; ++l) {
      span<const cbf16_t> row = data.get_view<static_cast<unsigned>(resource_grid_dimensions::symbol)>({l, p});
      std::memcpy(&out[(size_t(p) * MAX_NSYMB_PER_SLOT + l) * c.nof_subc * 2], row.data(), size_t(c.nof_subc) * 4);
    }
  }
  return out;
}

double time_map(const resource& r, unsigned nof_grid_ports, unsigned nof_subc)
{
  auto                  gen = make_generator("auto");
  grid_tensor           data({nof_subc, MAX_NSYMB_PER_SLOT, nof_grid_ports});
  std::atomic<unsigned> empty{0};
  resource_grid_writer_impl            writer(data, empty);
  const nzp_csi_rs_generator::config_t cfg = make_config(r);
  for (int i = 0; i < 20; ++i) {
    gen->map(writer, cfg);
  }
  const int  reps = 2000;
  const auto t0   = std::chrono::steady_clock::now();
  for (int i = 0; i < reps; ++i) {
    gen->map(writer, cfg);
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
  using cf = std::complex<float>;
  // resource: numerology, slot, start_rb, nof_rb, row, k_ref, l0, cdm, density, n_id, amplitude, weights, scalar, seed
  const std::vector<test_case> cases = {
      {"row1_bypass_52prb", 1, 624, {{1, 3, 0, 52, 1, {0}, 4, CDM_NONE, D_THREE, 41, 1.0F, W_SCALAR, cf(1, 0), 0}}},
      {"row1_grid_edge_cinit_wrap", 1, 3276,
       {{3, 79, 271, 2, 1, {3}, 13, CDM_NONE, D_THREE, 1023, 2.8F, W_SCALAR, cf(-1, 0), 0}}},
      {"row1_one_prb", 1, 624, {{1, 7, 7, 1, 1, {2}, 0, CDM_NONE, D_THREE, 500, 1.0F, W_SCALAR, cf(1, 0), 0}}},
      {"row1_273prb_weight", 1, 3276,
       {{1, 19, 0, 273, 1, {1}, 6, CDM_NONE, D_THREE, 7, 1.0F, W_SCALAR, cf(0.5F, -0.5F), 0}}},
      {"row2_even_density_even_start_last_prb", 1, 624,
       {{1, 2, 4, 47, 2, {11}, 0, CDM_NONE, D_EVEN, 100, 1.0F, W_SCALAR, cf(1, 0), 0}}},
      {"row2_even_density_odd_start", 1, 624,
       {{1, 2, 5, 47, 2, {11}, 0, CDM_NONE, D_EVEN, 101, 1.0F, W_SCALAR, cf(0, 1), 0}}},
      {"row2_odd_density_even_start", 1, 624,
       {{1, 2, 4, 47, 2, {11}, 0, CDM_NONE, D_ODD, 102, 0.5F, W_SCALAR, cf(1, 0), 0}}},
      {"row2_odd_density_odd_start", 1, 624,
       {{1, 2, 5, 47, 2, {11}, 0, CDM_NONE, D_ODD, 103, 1.0F, W_SCALAR, cf(-2, 0), 0}}},
      {"row2_one_prb_dot5", 1, 624, {{0, 9, 9, 1, 2, {5}, 3, CDM_NONE, D_ODD, 104, 1.0F, W_SCALAR, cf(1, 0), 0}}},
      {"row2_273prb", 1, 3276, {{1, 11, 0, 273, 2, {6}, 9, CDM_NONE, D_ONE, 105, 1.0F, W_SCALAR, cf(1, 0), 0}}},
      {"row3_identity_k10", 2, 624, {{1, 4, 0, 52, 3, {10}, 5, CDM_FD2, D_ONE, 200, 1.0F, W_IDENTITY, cf(), 0}}},
      {"row3_even_density_odd_start_weights", 2, 624,
       {{1, 5, 3, 45, 3, {4}, 7, CDM_FD2, D_EVEN, 201, 1.0F, W_SEEDED, cf(), 301}}},
      {"row3_odd_density_even_start_weights", 2, 624,
       {{1, 6, 6, 43, 3, {0}, 2, CDM_FD2, D_ODD, 202, 1.4F, W_SEEDED, cf(), 302}}},
      {"row4_identity_273prb", 4, 3276, {{1, 8, 0, 273, 4, {8}, 10, CDM_FD2, D_ONE, 300, 1.0F, W_IDENTITY, cf(), 0}}},
      {"row4_weights", 4, 624, {{1, 9, 3, 49, 4, {0}, 1, CDM_FD2, D_ONE, 301, 1.0F, W_SEEDED, cf(), 303}}},
      {"row5_identity_last_symbols", 4, 624,
       {{1, 10, 0, 52, 5, {10}, 12, CDM_FD2, D_ONE, 400, 1.0F, W_IDENTITY, cf(), 0}}},
      {"row5_permutation", 4, 1488,
       {{1, 12, 100, 24, 5, {3}, 5, CDM_FD2, D_ONE, 401, 1.0F, W_PERMUTATION, cf(4.9F, 0), 0}}},
      {"multi_trs_and_row4", 4, 624,
       {{1, 13, 0, 52, 1, {1}, 4, CDM_NONE, D_THREE, 33, 1.0F, W_SCALAR, cf(1, 0), 0},
        {1, 13, 0, 52, 1, {1}, 8, CDM_NONE, D_THREE, 33, 1.0F, W_SCALAR, cf(1, 0), 0},
        {1, 13, 0, 52, 4, {4}, 13, CDM_FD2, D_ONE, 34, 1.0F, W_IDENTITY, cf(), 0}}},
  };

  const bool  avx512     = cpu_supports_feature(cpu_feature::avx512f) && cpu_supports_feature(cpu_feature::avx512bw);
  const bool  avx2       = cpu_supports_feature(cpu_feature::avx2) && cpu_supports_feature(cpu_feature::fma);
  std::string auto_name  = avx512 ? "avx512" : (avx2 ? "avx2" : "generic");
  auto        gen_auto   = make_generator("auto");
  auto        gen_generic = make_generator("generic");

  npz_writer  npz;
  std::string names;
  for (size_t i = 0; i != cases.size(); ++i) {
    const test_case& c = cases[i];
    names += (i ? "\n" : "") + std::string(c.name);
    const std::vector<uint16_t> ga = run_case(c, *gen_auto);
    const std::vector<uint16_t> gg = run_case(c, *gen_generic);

    char key[16];
    std::snprintf(key, sizeof(key), "c%02zu_", i);
    const std::string    k = key;
    std::vector<int32_t> cfgv;
    std::vector<float>   amp, wv;
    unsigned             symbol_mask = 0;
    for (const resource& r : c.resources) {
      cfgv.insert(cfgv.end(), {int32_t(r.numerology), int32_t(r.slot_index), int32_t(r.start_rb), int32_t(r.nof_rb),
                               int32_t(r.row), int32_t(r.k_ref.size())});
      for (unsigned q = 0; q != 6; ++q) {
        cfgv.push_back(q < r.k_ref.size() ? int32_t(r.k_ref[q]) : 0);
      }
      cfgv.insert(cfgv.end(), {int32_t(r.l0), 0, int32_t(r.cdm), int32_t(r.density), int32_t(r.scrambling_id),
                               int32_t(c.nof_grid_ports), int32_t(c.nof_subc)});
      amp.push_back(r.amplitude);
      for (const cf& v : weights_of(r)) {
        wv.push_back(v.real());
        wv.push_back(v.imag());
      }
      for (const csi_rs_pattern_port& pp : pattern_of(r).prb_patterns) {
        symbol_mask |= unsigned(mask_of(pp.symbol_mask));
      }
    }
    std::vector<int32_t> symbols;
    for (unsigned l = 0; l != MAX_NSYMB_PER_SLOT; ++l) {
      if ((symbol_mask >> l) & 1u) {
        symbols.push_back(int32_t(l));
      }
    }
    // the reference writes no other symbol row
    std::vector<uint16_t> grid, gen_val;
    std::vector<int32_t>  gen_idx;
    size_t                nonzero = 0;
    for (unsigned p = 0; p != c.nof_grid_ports; ++p) {
      for (unsigned l = 0; l != MAX_NSYMB_PER_SLOT; ++l) {
        const size_t off    = (size_t(p) * MAX_NSYMB_PER_SLOT + l) * c.nof_subc * 2;
        const bool   stored = (symbol_mask >> l) & 1u;
        for (size_t q = 0; q != size_t(c.nof_subc) * 2; q += 2) {
          const bool nz = ga[off + q] != 0 || ga[off + q + 1] != 0 || gg[off + q] != 0 || gg[off + q + 1] != 0;
          if (nz && !stored) {
            std::fprintf(stderr, "%s: symbol %u written outside the pattern\n", c.name, l);
            return 1;
          }
          if (stored) {
            nonzero += nz;
            if (ga[off + q] != gg[off + q] || ga[off + q + 1] != gg[off + q + 1]) {
              gen_idx.push_back(int32_t(grid.size() / 2));
              gen_val.push_back(gg[off + q]);
              gen_val.push_back(gg[off + q + 1]);
            }
            grid.push_back(ga[off + q]);
            grid.push_back(ga[off + q + 1]);
          }
        }
      }
    }
    const size_t n_res = c.resources.size();
    npz.add<int32_t>(k + "cfg", cfgv, {n_res, 19});
    npz.add<float>(k + "amp", amp);
    npz.add<float>(k + "w", wv, {n_res, 4, 4, 2});
    npz.add<int32_t>(k + "symbols", symbols);
    npz.add<uint16_t>(k + "grid", grid, {c.nof_grid_ports, symbols.size(), c.nof_subc, 2});
    npz.add<int32_t>(k + "gen_idx", gen_idx);
    npz.add<uint16_t>(k + "gen_val", gen_val, {gen_idx.size(), 2});
    std::printf("%-40s ports %u subc %4u rows %zu written REs %6zu generic differs at %zu\n", c.name, c.nof_grid_ports,
                c.nof_subc, symbols.size(), nonzero, gen_idx.size());
  }
  npz.add<uint8_t>("names", std::vector<uint8_t>(names.begin(), names.end()));
  npz.add<uint8_t>("precoders", std::vector<uint8_t>(auto_name.begin(), auto_name.end()));

  // seeded valid configurations over rows 1-12
  static const unsigned nof_k[13] = {0, 1, 1, 1, 1, 1, 4, 2, 2, 6, 3, 4, 4};
  static const unsigned k_end[13] = {0, 4, 12, 11, 9, 11, 11, 11, 11, 11, 11, 11, 11};
  static const unsigned cdm[13]   = {0, CDM_NONE, CDM_NONE, CDM_FD2, CDM_FD2,     CDM_FD2, CDM_FD2,    CDM_FD2,
                                     CDM_FD2_TD2, CDM_FD2,  CDM_FD2_TD2, CDM_FD2, CDM_FD2_TD2};
  static const unsigned extra_l[13] = {0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1}; // symbols beyond l0
  std::mt19937_64      rng(7415);
  std::vector<int32_t> pin, pout;
  const unsigned       nof_patterns = 300;
  for (unsigned i = 0; i != nof_patterns; ++i) {
    resource r{};
    r.row = 1 + (i < 12 ? i : unsigned(rng() % 12));
    for (unsigned q = 0; q != nof_k[r.row]; ++q) {
      r.k_ref.push_back(unsigned(rng() % k_end[r.row]));
    }
    r.l0       = unsigned(rng() % (14 - extra_l[r.row]));
    r.cdm      = cdm[r.row];
    r.start_rb = unsigned(rng() % 200);
    r.nof_rb   = 1 + unsigned(rng() % 75);
    const bool dot5_ok = r.row == 2 || r.row == 3 || r.row == 11 || r.row == 12;
    r.density          = r.row == 1 ? D_THREE : (dot5_ok ? D_ONE + unsigned(rng() % 3) : D_ONE);
    const csi_rs_pattern p = pattern_of(r);
    pin.insert(pin.end(), {int32_t(r.start_rb), int32_t(r.nof_rb), int32_t(r.row), int32_t(r.k_ref.size())});
    for (unsigned q = 0; q != 6; ++q) {
      pin.push_back(q < r.k_ref.size() ? int32_t(r.k_ref[q]) : 0);
    }
    pin.insert(pin.end(), {int32_t(r.l0), 0, int32_t(r.cdm), int32_t(r.density)});
    pout.insert(pout.end(), {int32_t(p.rb_begin), int32_t(p.rb_end), int32_t(p.rb_stride), int32_t(p.prb_patterns.size())});
    for (unsigned q = 0; q != 16; ++q) {
      pout.push_back(q < p.prb_patterns.size() ? mask_of(p.prb_patterns[q].re_mask) : 0);
      pout.push_back(q < p.prb_patterns.size() ? mask_of(p.prb_patterns[q].symbol_mask) : 0);
    }
  }
  npz.add<int32_t>("pattern_in", pin, {nof_patterns, 14});
  npz.add<int32_t>("pattern_out", pout, {nof_patterns, 36});

  const resource t1  = {1, 0, 0, 273, 1, {0}, 4, CDM_NONE, D_THREE, 1, 1.0F, W_SCALAR, cf(1, 0), 0};
  const resource t4  = {1, 0, 0, 273, 4, {0}, 4, CDM_FD2, D_ONE, 1, 1.0F, W_IDENTITY, cf(), 0};
  const double   us1 = time_map(t1, 1, 3276), us4 = time_map(t4, 4, 3276);
  std::printf("reference map(), one thread, %s precoder: row 1 273 PRB %.2f us, row 4 273 PRB %.2f us\n",
              auto_name.c_str(), us1, us4);
  npz.add<double>("ref_map_us", {us1, us4});
  if (!npz.save(argv[1])) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  return 0;
}
