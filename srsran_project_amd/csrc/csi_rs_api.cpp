// csi_rs_api.cpp -- C-ABI of the MI355X NZP-CSI-RS generator (include/srsran_amd/csi_rs.h): get_csi_rs_pattern
// (lib/ran/csi_rs/csi_rs_pattern.cpp:34-499), the sequence geometry of nzp_csi_rs_generator_impl.cpp:72-173, the
// validation the reference leaves to assertions, and the single launch of csi_rs.hip.
#include "srsran_amd/csi_rs.h"
#include "srsran_amd/ldpc.h"

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "csi_rs_args.h"
#include "device_buffer.h"
#include "gold_sequence.h"
#include "staged_call.h"
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

using namespace srs_amd;

namespace {

constexpr uint32_t NRE = 12;

enum : uint32_t { CDM_NONE = 0, CDM_FD2 = 1, CDM_FD2_TD2 = 2, CDM_FD2_TD4 = 3 };
enum : uint32_t { DENSITY_THREE = 0, DENSITY_ONE = 1, DENSITY_DOT5_EVEN = 2, DENSITY_DOT5_ODD = 3 };

// TS 38.211 Table 7.4.1.5.3-1, rows 1-12, as the reference's mapping_row_N functions state it.
struct row_info {
  uint32_t nof_ports;
  uint32_t nof_k_ref;
  uint32_t k_end;     // every k_ref below this
  uint32_t cdm;
  bool     dot5;      // density 0.5 allowed beside density one
};
constexpr row_info ROWS[13] = {
    {},
    {1, 1, 4, CDM_NONE, false}, // density three only
    {1, 1, NRE, CDM_NONE, true},
    {2, 1, NRE - 1, CDM_FD2, true},
    {4, 1, NRE - 3, CDM_FD2, false},
    {4, 1, NRE - 1, CDM_FD2, false},
    {8, 4, NRE - 1, CDM_FD2, false},
    {8, 2, NRE - 1, CDM_FD2, false},
    {8, 2, NRE - 1, CDM_FD2_TD2, false},
    {12, 6, NRE - 1, CDM_FD2, false},
    {12, 3, NRE - 1, CDM_FD2_TD2, false},
    {16, 4, NRE - 1, CDM_FD2, true},
    {16, 4, NRE - 1, CDM_FD2_TD2, true},
};

bool is_dot5(uint32_t density)
{
  return density == DENSITY_DOT5_EVEN || density == DENSITY_DOT5_ODD;
}

// k_bar and l_bar of `port` (mapping_row_1 .. mapping_row_12).
void port_reference(const srs_amd_csi_rs_config& c, uint32_t port, uint32_t& k_bar, uint32_t& l_bar)
{
  const uint32_t* k  = c.k_ref;
  const uint32_t  l0 = c.symbol_l0;
  const uint32_t  g2 = port / 2; // fd-CDM2 group
  const uint32_t  g4 = port / 4; // cdm4-FD2-TD2 group
  switch (c.row) {
    case 4:
      k_bar = k[0] + 2 * g2, l_bar = l0;
      break;
    case 5:
      k_bar = k[0], l_bar = l0 + g2;
      break;
    case 6:
    case 9:
      k_bar = k[g2], l_bar = l0;
      break;
    case 7:
      k_bar = k[g2 % 2], l_bar = l0 + g2 / 2;
      break;
    case 8:
    case 10:
    case 12:
      k_bar = k[g4], l_bar = l0;
      break;
    case 11:
      k_bar = k[g2 % 4], l_bar = l0 + g2 / 4;
      break;
    default: // rows 1, 2, 3
      k_bar = k[0], l_bar = l0;
      break;
  }
}

int derive_pattern(const srs_amd_csi_rs_config& c, srs_amd_csi_rs_pattern_desc& out)
{
  if (c.row == 0 || c.row > 18) {
    return fail(SRS_AMD_EINVAL, "Invalid mapping table row.");
  }
  if (c.row > 12) {
    return fail(SRS_AMD_EINVAL, "Unsupported mapping table row");
  }
  const row_info& row = ROWS[c.row];
  if (c.nof_k_ref != row.nof_k_ref) {
    return fail(SRS_AMD_EINVAL, "CSI-RS Mapping Row %u: %u k_ref are needed", c.row, row.nof_k_ref);
  }
  for (uint32_t i = 0; i != row.nof_k_ref; ++i) {
    if (c.k_ref[i] >= row.k_end) {
      return fail(SRS_AMD_EINVAL, "CSI-RS Mapping Row %u: k references outside of the valid range", c.row);
    }
  }
  const bool density_ok = c.row == 1 ? c.freq_density == DENSITY_THREE
                                     : (c.freq_density == DENSITY_ONE || (row.dot5 && is_dot5(c.freq_density)));
  if (!density_ok) {
    return fail(SRS_AMD_EINVAL, "CSI-RS Mapping Row %u: invalid density", c.row);
  }
  if (c.cdm != row.cdm) {
    return fail(SRS_AMD_EINVAL, "CSI-RS Mapping Row %u: invalid CDM type", c.row);
  }
  std::memset(&out, 0, sizeof(out));
  // build_re_patterns (csi_rs_pattern.cpp:371-436)
  out.rb_begin  = c.start_rb;
  out.rb_end    = c.start_rb + c.nof_rb;
  out.rb_stride = 1;
  if (is_dot5(c.freq_density)) {
    out.rb_stride = 2;
    if ((c.start_rb % 2 != 0) == (c.freq_density == DENSITY_DOT5_EVEN)) {
      ++out.rb_begin;
    }
  }
  out.nof_ports            = row.nof_ports;
  const uint32_t nof_symb  = c.cdm == CDM_FD2_TD2 ? 2 : (c.cdm == CDM_FD2_TD4 ? 4 : 1);
  for (uint32_t p = 0; p != row.nof_ports; ++p) {
    uint32_t k_bar = 0, l_bar = 0;
    port_reference(c, p, k_bar, l_bar);
    if (l_bar + nof_symb > 14 || l_bar + nof_symb < l_bar) {
      return fail(SRS_AMD_EINVAL, "CSI-RS Mapping Row %u: symbol %u outside the slot.", c.row, l_bar + nof_symb - 1);
    }
    uint32_t re = 1u << k_bar;
    if (c.row == 1) {
      re |= (1u << (k_bar + 4)) | (1u << (k_bar + 8));
    } else if (c.cdm != CDM_NONE) {
      re |= 1u << (k_bar + 1);
    }
    out.port[p].re_mask     = static_cast<uint16_t>(re);
    out.port[p].symbol_mask = static_cast<uint16_t>(((1u << nof_symb) - 1u) << l_bar);
  }
  return SRS_AMD_OK;
}

struct derived {
  srs_amd_csi_rs_pattern_desc pattern;
  uint32_t                    skip_bits;
  uint32_t                    seq_len;
  uint32_t                    group_size, nof_groups, per_prb;
  float                       amplitude;
};

// TS 38.211 7.4.1.5.2; the reference's 32-bit product wraps (numerology 3, slot 79, n_id 1023), which the final
// mod 2^31 makes harmless: computed here mod 2^31 in 64 bits.
uint32_t c_init_of(uint32_t slot_index, uint32_t symbol, uint32_t n_id)
{
  const uint64_t v = (static_cast<uint64_t>(1024) * (14u * slot_index + symbol + 1u) * (2u * n_id + 1u) + n_id);
  return static_cast<uint32_t>(v & 0x7fffffffu);
}

int derive(const srs_amd_csi_rs_config& c, uint32_t nof_grid_ports, uint32_t nof_subc, derived& d)
{
  int rc = derive_pattern(c, d.pattern);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  if (c.row > 5) {
    return fail(SRS_AMD_EINVAL,
                "CSI-RS row %u has %u ports: mapping supports rows 1 to 5 only (at most %u precoding ports).", c.row,
                d.pattern.nof_ports, CSI_RS_MAX_PORTS);
  }
  if (d.pattern.nof_ports > nof_grid_ports) {
    return fail(SRS_AMD_EINVAL, "The precoding number of ports (i.e., %u) exceeds the grid number of ports (i.e., %u).",
                d.pattern.nof_ports, nof_grid_ports);
  }
  if (c.symbol_l0 >= 14) {
    return fail(SRS_AMD_EINVAL, "CSI-RS Mapping: l_0, i.e., %u outside the valid range, i.e., [0, 14).", c.symbol_l0);
  }
  if (c.nof_rb == 0 || c.start_rb > SRS_AMD_MAX_RB || c.nof_rb > SRS_AMD_MAX_RB ||
      static_cast<uint64_t>(c.start_rb + c.nof_rb) * NRE > nof_subc) {
    return fail(SRS_AMD_EINVAL, "CSI-RS PRBs [%u, %u) do not fit a grid of %u subcarriers.", c.start_rb,
                c.start_rb + c.nof_rb, nof_subc);
  }
  if (d.pattern.rb_begin >= d.pattern.rb_end) {
    return fail(SRS_AMD_EINVAL, "At least one subcarrier must be used by the allocation pattern.");
  }
  if (c.scrambling_id > 1023) {
    return fail(SRS_AMD_EINVAL, "CSI-RS scrambling identifier (i.e., %u) exceeds 1023.", c.scrambling_id);
  }
  if (c.numerology > 4 || c.slot_index >= (10u << c.numerology)) {
    return fail(SRS_AMD_EINVAL, "Slot index %u is outside the frame of numerology %u.", c.slot_index, c.numerology);
  }
  // get_nof_skipped_elements (:72-109): the elements of the PRBs below the first occupied one
  const uint32_t first_prb = d.pattern.rb_begin;
  uint32_t       advance   = 0;
  if (c.freq_density == DENSITY_THREE) {
    advance = 3 * first_prb;
  } else if (c.freq_density == DENSITY_ONE) {
    advance = c.row == 2 ? first_prb : 2 * first_prb;
  } else {
    advance = c.row == 2 ? first_prb / 2 : first_prb;
  }
  d.skip_bits = 2 * advance;
  // get_seq_len (:142-173): its rounding branches count the PRBs of the stride in [rb_begin, rb_end)
  const uint32_t occupied = (d.pattern.rb_end - d.pattern.rb_begin + d.pattern.rb_stride - 1) / d.pattern.rb_stride;
  d.group_size            = c.cdm == CDM_NONE ? 1 : 2;
  d.nof_groups            = d.pattern.nof_ports / d.group_size;
  d.per_prb               = c.row == 1 ? 3 : d.group_size;
  d.seq_len               = occupied * d.per_prb;
  d.amplitude             = static_cast<float>(M_SQRT1_2 * static_cast<double>(c.amplitude));
  return SRS_AMD_OK;
}

} // namespace

struct srs_amd_csi_rs_generator {
  int           device = 0;
  hipStream_t   stream = nullptr; // host form
  uint32_t*     d_jump = nullptr;
  device_buffer descriptors;
  device_buffer host_io;
  pinned_stage  stage;
  stream_order  order;
  std::mutex    mtx;
  std::mutex    host_mtx; // the host form's buffer and stream

  ~srs_amd_csi_rs_generator()
  {
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    (void)hipFree(d_jump);
  }
};

extern "C" {

int srs_amd_csi_rs_pattern(const srs_amd_csi_rs_config* cfg, srs_amd_csi_rs_pattern_desc* out)
{
  if (cfg == nullptr || out == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  srs_amd_csi_rs_pattern_desc p{};
  const int              rc = derive_pattern(*cfg, p);
  if (rc == SRS_AMD_OK) {
    *out = p;
  }
  return rc;
}

int srs_amd_csi_rs_reserved(const srs_amd_csi_rs_config* cfg, srs_amd_re_pattern* patterns, uint32_t* nof_patterns)
{
  if (cfg == nullptr || patterns == nullptr || nof_patterns == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  *nof_patterns = 0;
  srs_amd_csi_rs_pattern_desc p{};
  const int              rc = derive_pattern(*cfg, p);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  if (cfg->start_rb > SRS_AMD_MAX_RB || cfg->nof_rb > SRS_AMD_MAX_RB || p.rb_end > SRS_AMD_MAX_RB) {
    return fail(SRS_AMD_EINVAL, "CSI-RS PRBs [%u, %u) exceed %u.", cfg->start_rb, cfg->start_rb + cfg->nof_rb,
                SRS_AMD_MAX_RB);
  }
  srs_amd_re_pattern base;
  std::memset(&base, 0, sizeof(base));
  for (uint32_t rb = p.rb_begin; rb < p.rb_end; rb += p.rb_stride) {
    base.crb_mask[rb / 8] |= static_cast<uint8_t>(1u << (rb % 8));
  }
  uint32_t n = 0;
  for (uint32_t port = 0; port != p.nof_ports; ++port) {
    bool seen = false;
    for (uint32_t i = 0; i != n && !seen; ++i) {
      seen = patterns[i].re_mask == p.port[port].re_mask && patterns[i].symbols == p.port[port].symbol_mask;
    }
    if (seen) {
      continue;
    }
    if (n == SRS_AMD_MAX_RE_PATTERNS) {
      return fail(SRS_AMD_EINVAL, "More than %u distinct CSI-RS RE patterns.", SRS_AMD_MAX_RE_PATTERNS);
    }
    patterns[n]         = base;
    patterns[n].re_mask = p.port[port].re_mask;
    patterns[n].symbols = p.port[port].symbol_mask;
    ++n;
  }
  *nof_patterns = n;
  return SRS_AMD_OK;
}

int srs_amd_csi_rs_validate(const srs_amd_csi_rs_config* cfg, uint32_t nof_grid_ports, uint32_t nof_subc)
{
  if (cfg == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  return derive(*cfg, nof_grid_ports, nof_subc, d);
}

int srs_amd_csi_rs_generator_create(srs_amd_csi_rs_generator** gen, int device)
{
  if (gen == nullptr) {
    return fail(SRS_AMD_EINVAL, "null handle pointer");
  }
  *gen   = nullptr;
  int rc = select_device(device);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  auto* g                 = new srs_amd_csi_rs_generator();
  g->device               = device;
  std::vector<uint32_t> j = gold_jump_tables();
  hipError_t            e = hipMalloc(reinterpret_cast<void**>(&g->d_jump), j.size() * sizeof(uint32_t));
  if (e == hipSuccess) {
    e = hipMemcpy(g->d_jump, j.data(), j.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
  }
  if (e != hipSuccess) {
    delete g;
    return hip_fail(e, "CSI-RS generator tables");
  }
  *gen = g;
  return SRS_AMD_OK;
}

void srs_amd_csi_rs_generator_destroy(srs_amd_csi_rs_generator* gen)
{
  delete gen;
}

int srs_amd_csi_rs_map_slot(srs_amd_csi_rs_generator*    gen,
                            const srs_amd_csi_rs_config* cfgs,
                            uint32_t                     nof_resources,
                            uint32_t*                    d_grids,
                            uint64_t                     grid_stride,
                            uint32_t                     nof_grids,
                            uint32_t                     nof_grid_ports,
                            uint32_t                     nof_subc,
                            void*                        stream)
{
  if (gen == nullptr) {
    return fail(SRS_AMD_EINVAL, "null CSI-RS generator");
  }
  if (nof_resources == 0) {
    return SRS_AMD_OK;
  }
  if (cfgs == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  if ((reinterpret_cast<uintptr_t>(d_grids) & 3u) != 0) {
    return fail(SRS_AMD_EINVAL, "misaligned device buffer");
  }
  if (nof_resources > 65535u) {
    return fail(SRS_AMD_EINVAL, "More than 65535 resources (i.e., %u) in one call.", nof_resources);
  }
  if (nof_grid_ports == 0 || nof_subc == 0 ||
      (nof_grids > 1 && grid_stride < static_cast<uint64_t>(nof_grid_ports) * CSI_RS_NSYMB * nof_subc)) {
    return fail(SRS_AMD_EINVAL, "Invalid grid geometry (%u ports, %u subcarriers, stride %llu).", nof_grid_ports,
                nof_subc, static_cast<unsigned long long>(grid_stride));
  }
  // validate every resource before anything is launched
  std::vector<csi_rs_item> items;
  items.reserve(2 * static_cast<size_t>(nof_resources));
  for (uint32_t i = 0; i != nof_resources; ++i) {
    const srs_amd_csi_rs_config& c = cfgs[i];
    if (c.d_grid == nullptr && (d_grids == nullptr || c.grid >= nof_grids)) {
      return fail(SRS_AMD_EINVAL, "grid index %u out of range (or no grid).", c.grid);
    }
    if ((reinterpret_cast<uintptr_t>(c.d_grid) & 3u) != 0) {
      return fail(SRS_AMD_EINVAL, "misaligned device buffer");
    }
    derived   d{};
    const int rc = derive(c, nof_grid_ports, nof_subc, d);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    // the mapper's bypass (resource_grid_mapper_impl.cpp:246-247): one layer, one port, coefficient == 1.0F
    const bool bypass = d.pattern.nof_ports == 1 && c.weights[0][0][0] == 1.0F && c.weights[0][0][1] == 0.0F;
    for (uint32_t g = 0; g != d.nof_groups; ++g) {
      const uint32_t                     port = g * d.group_size;
      const srs_amd_csi_rs_pattern_port& pp   = d.pattern.port[port];
      csi_rs_item                        o;
      std::memset(&o, 0, sizeof(o));
      o.grid       = c.d_grid != nullptr ? c.d_grid : d_grids + c.grid * grid_stride;
      o.symbol     = static_cast<uint32_t>(__builtin_ctz(pp.symbol_mask));
      o.c_init     = c_init_of(c.slot_index, o.symbol, c.scrambling_id);
      o.skip_bits  = d.skip_bits;
      o.seq_len    = d.seq_len;
      o.first_subc = d.pattern.rb_begin * NRE;
      o.prb_step   = d.pattern.rb_stride * NRE;
      o.per_prb    = d.per_prb;
      o.k_bar      = static_cast<uint32_t>(__builtin_ctz(pp.re_mask));
      o.k_step     = c.row == 1 ? 4 : 1;
      o.nof_subc   = nof_subc;
      o.group_size = d.group_size;
      o.nof_tx     = d.pattern.nof_ports;
      o.bypass     = bypass ? 1 : 0;
      o.amplitude  = d.amplitude;
      for (uint32_t q = 0; q != d.group_size; ++q) {
        for (uint32_t t = 0; t != d.pattern.nof_ports; ++t) {
          o.w[q][t][0] = c.weights[port + q][t][0];
          o.w[q][t][1] = c.weights[port + q][t][1];
        }
      }
      items.push_back(o);
    }
  }

  hipStream_t                 s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(gen->mtx);
  const size_t                bytes = items.size() * sizeof(csi_rs_item);
  staged_call call("CSI-RS generator", gen->device, gen->descriptors, bytes, gen->stage, bytes, gen->order, s);
  if (!call.ok()) {
    return call.finish();
  }
  std::memcpy(call.host(), items.data(), bytes);
  hipError_t e = call.upload(gen->descriptors.ptr, bytes);
  if (e == hipSuccess) {
    e = launch_csi_rs_map(gen->descriptors.as<csi_rs_item>(), static_cast<uint32_t>(items.size()), gen->d_jump, s);
  }
  return call.finish(e);
}

int srs_amd_csi_rs_map(srs_amd_csi_rs_generator*    gen,
                       const srs_amd_csi_rs_config* cfg,
                       uint32_t*                    grid,
                       uint32_t                     nof_ports,
                       uint32_t                     nof_subc)
{
  if (gen == nullptr || cfg == nullptr || grid == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  int     rc = derive(*cfg, nof_ports, nof_subc, d);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  const size_t bytes = static_cast<size_t>(nof_ports) * CSI_RS_NSYMB * nof_subc * sizeof(uint32_t);
  host_call    call("CSI-RS generator", gen->host_mtx, gen->device, gen->stream);
  call.grow(gen->host_io, bytes);
  call.in(gen->host_io.ptr, grid, bytes);
  if (!call.ok()) {
    return call.finish();
  }
  srs_amd_csi_rs_config c = *cfg;
  c.grid                  = 0;
  c.d_grid                = nullptr;
  rc = srs_amd_csi_rs_map_slot(gen, &c, 1, gen->host_io.as<uint32_t>(), 0, 1, nof_ports, nof_subc, gen->stream);
  if (rc == SRS_AMD_OK) {
    call.out(grid, gen->host_io.ptr, bytes);
  }
  return call.finish(rc);
}


} // extern "C"
