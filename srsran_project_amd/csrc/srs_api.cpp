// srs_api.cpp -- C-ABI of the MI355X SRS channel estimator (include/srsran_amd/srs.h): get_srs_information
// (lib/ran/srs/srs_information.cpp:38-103), the validation of srs_validator_generic_impl.cpp, the search range of
// time_alignment_estimator_dft_impl::estimate_ta_correlation (:245-263), the base-sequence cache and the launch
// sequence of srs.hip.
#include "srsran_amd/srs.h"
#include "srsran_amd/ldpc.h"
#include "srsran_amd/low_papr.h"

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "device_buffer.h"
#include "dft_engine.h"
#include "srs_args.h"
#include "staged_call.h"
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace srs_amd;

namespace {

#include "srs_tables.inc"

constexpr double   T_C        = 1.0 / (480000.0 * 4096.0); // TS 38.211 Section 4.1
constexpr uint32_t N_RB_SC    = 12;
constexpr uint32_t MAX_NOF_RE = 275 * 12; // time_alignment_estimator_dft_impl::max_nof_re

constexpr uint32_t IDFT_SIZES[] = {
#define SRS_SIZE(NN) NN,
    SRS_SRS_FOR_EACH_SIZE(SRS_SIZE)
#undef SRS_SIZE
};
constexpr uint32_t NOF_IDFT_SIZES = sizeof(IDFT_SIZES) / sizeof(IDFT_SIZES[0]);

int size_slot(uint32_t N)
{
  for (uint32_t i = 0; i != NOF_IDFT_SIZES; ++i) {
    if (IDFT_SIZES[i] == N) {
      return static_cast<int>(i);
    }
  }
  return -1;
}

// time_alignment_estimator_dft_impl::get_idft (:226-243): min_dft_size 128, max_dft_size 4096
uint32_t idft_size_of(uint32_t M)
{
  const uint32_t need = (M * 4096u) / MAX_NOF_RE;
  uint32_t       n    = 128;
  while (n < need) {
    n *= 2;
  }
  return n;
}

bool one_two_four(uint32_t v)
{
  return v == 1 || v == 2 || v == 4;
}

// The resource checks shared by every entry point; fills the information of `antenna_port`.
int derive_information(const srs_amd_srs_config& c, uint32_t antenna_port, srs_amd_srs_information& info)
{
  if (!one_two_four(c.nof_antenna_ports) || !one_two_four(c.nof_symbols)) {
    return fail(SRS_AMD_EINVAL, "The number of antenna ports (i.e., %u) and of symbols (i.e., %u) must be 1, 2 or 4.",
                c.nof_antenna_ports, c.nof_symbols);
  }
  if (c.start_symbol + static_cast<uint64_t>(c.nof_symbols) > SRS_NSYMB) {
    return fail(SRS_AMD_EINVAL,
                "The start symbol index (i.e., %u) plus the number of symbols (i.e., %u) exceeds the number of symbols "
                "per slot (i.e., %u)",
                c.start_symbol, c.nof_symbols, SRS_NSYMB);
  }
  if (c.comb_size != 2 && c.comb_size != 4) {
    return fail(SRS_AMD_EINVAL, "Invalid comb size (i.e., %u).", c.comb_size);
  }
  // srs_resource_configuration::is_valid
  if (c.comb_offset >= c.comb_size || c.cyclic_shift > (c.comb_size == 2 ? 7u : 11u)) {
    return fail(SRS_AMD_EINVAL, "Invalid SRS resource configuration.");
  }
  if (c.configuration_index > 63 || c.bandwidth_index > 3) {
    return fail(SRS_AMD_EINVAL, "Invalid combination of c-SRS (i.e., %u) and b-SRS (i.e., %u)", c.configuration_index,
                c.bandwidth_index);
  }
  if (c.freq_hopping > 3 || c.freq_hopping < c.bandwidth_index) {
    return fail(SRS_AMD_EINVAL, "The SRS estimator does not support frequency hopping.");
  }
  if (c.hopping != 0) {
    return fail(SRS_AMD_EINVAL, "The SRS estimator does not support group or sequence hopping.");
  }
  if (c.sequence_id > 1023 || c.freq_position > 67 || c.freq_shift > 268 || c.numerology > 4) {
    return fail(SRS_AMD_EINVAL, "SRS resource field out of range (sequence_id %u, freq_position %u, freq_shift %u, numerology %u).",
                c.sequence_id, c.freq_position, c.freq_shift, c.numerology);
  }
  if (antenna_port >= c.nof_antenna_ports) {
    return fail(SRS_AMD_EINVAL, "Antenna port %u of %u.", antenna_port, c.nof_antenna_ports);
  }
  const srs_bandwidth_row& row  = SRS_BANDWIDTH_TABLE[c.configuration_index];
  const uint32_t           comb = c.comb_size;
  info.sequence_length          = (row.m_srs[c.bandwidth_index] * N_RB_SC) / comb;
  info.sequence_group           = c.sequence_id % 30; // f_gh = 0
  info.sequence_number          = 0;
  info.n_cs_max                 = comb == 4 ? 12 : 8;
  info.n_cs     = (c.cyclic_shift + (info.n_cs_max * antenna_port) / c.nof_antenna_ports) % info.n_cs_max;
  uint32_t k_tc = c.comb_offset;
  if (c.cyclic_shift >= info.n_cs_max / 2 && c.nof_antenna_ports == 4 && (antenna_port == 1 || antenna_port == 3)) {
    k_tc = (k_tc + comb / 2) % comb;
  }
  uint32_t k0 = c.freq_shift * N_RB_SC + k_tc;
  for (uint32_t b = 0; b <= c.bandwidth_index; ++b) {
    const uint32_t M_b = (row.m_srs[b] * N_RB_SC) / comb;
    const uint32_t n_b = ((4 * c.freq_position) / row.m_srs[b]) % row.N[b];
    k0 += comb * M_b * n_b;
  }
  info.mapping_initial_subcarrier = k0;
  info.comb_size                  = comb;
  info.idft_size                  = idft_size_of(info.sequence_length);
  if (!srs_amd_low_papr_length_valid(info.sequence_length) || size_slot(info.idft_size) < 0) {
    return fail(SRS_AMD_EINVAL, "Invalid sequence length %u.", info.sequence_length);
  }
  return SRS_AMD_OK;
}

struct derived {
  srs_amd_srs_information info[SRS_MAX_PORTS];
  uint32_t                max_ta_samples;
  uint32_t                scs_khz;
  double                  sampling_rate;
};

int derive(const srs_amd_srs_config& c, uint32_t nof_grid_ports, uint32_t nof_subc, derived& d)
{
  int rc = derive_information(c, 0, d.info[0]);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  for (uint32_t p = 1; p < c.nof_antenna_ports; ++p) {
    rc = derive_information(c, p, d.info[p]);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
  }
  if (c.nof_rx_ports == 0) {
    return fail(SRS_AMD_EINVAL, "Empty list of Rx ports for the SRS estimator.");
  }
  if (c.nof_rx_ports > SRS_MAX_PORTS) {
    return fail(SRS_AMD_EINVAL, "The number of receive ports (i.e., %u) exceeds the maximum (i.e., %u).", c.nof_rx_ports,
                SRS_MAX_PORTS);
  }
  for (uint32_t r = 0; r != c.nof_rx_ports; ++r) {
    if (c.rx_ports[r] >= nof_grid_ports) {
      return fail(SRS_AMD_EINVAL, "Rx port %u is outside the grid of %u ports.", c.rx_ports[r], nof_grid_ports);
    }
  }
  for (uint32_t p = 0; p != c.nof_antenna_ports; ++p) {
    const srs_amd_srs_information& info = d.info[p];
    if (info.mapping_initial_subcarrier + static_cast<uint64_t>(info.sequence_length - 1) * info.comb_size >= nof_subc) {
      return fail(SRS_AMD_EINVAL, "SRS resource exceeds maximum bandwidth.");
    }
  }
  // estimate_ta_correlation (:250-263) with stride = comb and max_ta = 1 / (n_cs_max scs comb)
  // (srs_estimator_generic_impl.cpp:109), in double as there
  d.scs_khz                  = 15u << c.numerology;
  const uint32_t N           = d.info[0].idft_size;
  const double   half_cp     = static_cast<double>((144u * 64u) >> (c.numerology + 1)) * T_C;
  d.sampling_rate            = static_cast<double>(static_cast<uint64_t>(N) * d.scs_khz * 1000u * c.comb_size);
  const double   max_ta      = 1.0 / static_cast<double>(d.info[0].n_cs_max * d.scs_khz * 1000u * c.comb_size);
  uint32_t       max_samples = static_cast<uint32_t>(std::floor(half_cp * d.sampling_rate));
  if (std::isnormal(max_ta)) {
    max_samples = std::min(max_samples, static_cast<uint32_t>(std::floor(max_ta * d.sampling_rate)));
  }
  if (max_samples == 0 || max_samples > N / 8) {
    return fail(SRS_AMD_EINVAL, "Time alignment range of %u samples does not fit the IDFT size %u.", max_samples, N);
  }
  d.max_ta_samples = max_samples;
  return SRS_AMD_OK;
}

// W_N^m = exp(-2*pi*i*m/N), double precision rounded to float (dft_engine.h).
std::vector<float2> twiddle_table(uint32_t N)
{
  std::vector<float2> t(N);
  for (uint32_t m = 0; m != N; ++m) {
    const double a = -2.0 * M_PI * static_cast<double>(m) / static_cast<double>(N);
    t[m]           = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
  }
  return t;
}

// complex_exponential_table(size, 1.0F) (include/srsran/phy/support/complex_exponential_table.h:43-49), appended to t
void append_cexp_table(std::vector<float2>& t, uint32_t size)
{
  for (uint32_t n = 0; n != size; ++n) {
    const std::complex<float> x =
        std::polar(1.0F, static_cast<float>(2 * M_PI) * static_cast<float>(n) / static_cast<float>(size));
    t.push_back(make_float2(x.real(), x.imag()));
  }
}

} // namespace

struct srs_amd_srs_estimator {
  int                         device = 0;
  hipStream_t                 stream = nullptr; // host form
  float2*                     d_tables = nullptr; // 1024-entry phase table, then the 24-entry cyclic-shift table
  float2*                     d_twiddles[NOF_IDFT_SIZES] = {};
  std::map<uint32_t, float2*> sequences; // (M << 8 | u) -> r_{u,0} in device memory
  device_buffer               descriptors;
  device_buffer               partials;
  device_buffer               host_io;
  pinned_stage                stage;
  stream_order                order;
  std::mutex                  mtx;
  std::mutex                  host_mtx; // the host form's buffer and stream

  ~srs_amd_srs_estimator()
  {
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    (void)hipFree(d_tables);
    for (float2* t : d_twiddles) {
      (void)hipFree(t);
    }
    for (auto& s : sequences) {
      (void)hipFree(s.second);
    }
  }

  // The base sequence r_{u,0} of length M, generated on the host and uploaded (blocking copy: complete before any
  // later launch on any stream) the first time it is met.
  int sequence(uint32_t M, uint32_t u, const float2*& out)
  {
    const uint32_t key = (M << 8) | u;
    auto           it  = sequences.find(key);
    if (it != sequences.end()) {
      out = it->second;
      return SRS_AMD_OK;
    }
    std::vector<float> r(2 * static_cast<size_t>(M));
    const int          rc = srs_amd_low_papr_sequence(r.data(), M, u, 0);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    float2*    p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), r.size() * sizeof(float));
    if (e == hipSuccess) {
      e = hipMemcpy(p, r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      (void)hipFree(p);
      return hip_fail(e, "SRS base sequence upload");
    }
    sequences.emplace(key, p);
    out = p;
    return SRS_AMD_OK;
  }
};

extern "C" {

int srs_amd_srs_bandwidth(uint32_t c_srs, uint32_t b_srs, uint32_t* m_srs, uint32_t* N)
{
  if (m_srs == nullptr || N == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  if (c_srs > 63 || b_srs > 3) {
    return fail(SRS_AMD_EINVAL, "Invalid combination of c-SRS (i.e., %u) and b-SRS (i.e., %u)", c_srs, b_srs);
  }
  *m_srs = SRS_BANDWIDTH_TABLE[c_srs].m_srs[b_srs];
  *N     = SRS_BANDWIDTH_TABLE[c_srs].N[b_srs];
  return SRS_AMD_OK;
}

int srs_amd_srs_get_information(const srs_amd_srs_config* config, uint32_t antenna_port, srs_amd_srs_information* info)
{
  if (config == nullptr || info == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  srs_amd_srs_information i{};
  const int               rc = derive_information(*config, antenna_port, i);
  if (rc == SRS_AMD_OK) {
    *info = i;
  }
  return rc;
}

int srs_amd_srs_validate(const srs_amd_srs_config* config, uint32_t nof_grid_ports, uint32_t nof_subc)
{
  if (config == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  return derive(*config, nof_grid_ports, nof_subc, d);
}

int srs_amd_srs_estimator_create(srs_amd_srs_estimator** est, int device)
{
  if (est == nullptr) {
    return fail(SRS_AMD_EINVAL, "null handle pointer");
  }
  *est   = nullptr;
  int rc = select_device(device);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  auto* d      = new srs_amd_srs_estimator();
  d->device    = device;
  hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    std::vector<float2> t;
    append_cexp_table(t, SRS_CEXP_TABLE_SIZE);
    append_cexp_table(t, SRS_CS_TABLE_SIZE);
    e = hipMalloc(reinterpret_cast<void**>(&d->d_tables), t.size() * sizeof(float2));
    if (e == hipSuccess) {
      e = hipMemcpy(d->d_tables, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
    }
  }
  for (uint32_t i = 0; i != NOF_IDFT_SIZES && e == hipSuccess; ++i) {
    const std::vector<float2> t = twiddle_table(IDFT_SIZES[i]);
    e                           = hipMalloc(reinterpret_cast<void**>(&d->d_twiddles[i]), t.size() * sizeof(float2));
    if (e == hipSuccess) {
      e = hipMemcpy(d->d_twiddles[i], t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
    }
  }
  if (e != hipSuccess) {
    delete d;
    return hip_fail(e, "SRS estimator tables");
  }
  *est = d;
  return SRS_AMD_OK;
}

void srs_amd_srs_estimator_destroy(srs_amd_srs_estimator* est)
{
  delete est;
}

int srs_amd_srs_estimate_batch(srs_amd_srs_estimator*    est,
                               const srs_amd_srs_config* configs,
                               uint32_t                  nof_pdus,
                               const uint32_t*           d_grids,
                               uint64_t                  grid_stride,
                               uint32_t                  nof_grids,
                               uint32_t                  nof_grid_ports,
                               uint32_t                  nof_subc,
                               srs_amd_srs_result*       d_results,
                               void*                     stream)
{
  if (est == nullptr) {
    return fail(SRS_AMD_EINVAL, "null SRS estimator");
  }
  if (nof_pdus == 0) {
    return SRS_AMD_OK;
  }
  if (configs == nullptr || d_results == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  if ((reinterpret_cast<uintptr_t>(d_grids) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0) {
    return fail(SRS_AMD_EINVAL, "misaligned device buffer");
  }
  if (nof_pdus > 65535u) {
    return fail(SRS_AMD_EINVAL, "More than 65535 PDUs (i.e., %u) in one batch.", nof_pdus);
  }
  if (nof_grid_ports == 0 || nof_subc == 0 ||
      (nof_grids > 1 && grid_stride < static_cast<uint64_t>(nof_grid_ports) * SRS_NSYMB * nof_subc)) {
    return fail(SRS_AMD_EINVAL, "Invalid grid geometry (%u ports, %u subcarriers, stride %llu).", nof_grid_ports, nof_subc,
                static_cast<unsigned long long>(grid_stride));
  }
  // validate every PDU before anything is launched
  std::vector<derived> geo(nof_pdus);
  for (uint32_t i = 0; i != nof_pdus; ++i) {
    const srs_amd_srs_config& c = configs[i];
    if (c.d_grid == nullptr && (d_grids == nullptr || c.grid >= nof_grids)) {
      return fail(SRS_AMD_EINVAL, "grid index %u out of range (or no grid).", c.grid);
    }
    if ((reinterpret_cast<uintptr_t>(c.d_grid) & 3u) != 0) {
      return fail(SRS_AMD_EINVAL, "misaligned device buffer");
    }
    const int rc = derive(c, nof_grid_ports, nof_subc, geo[i]);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
  }
  // PDUs grouped by IDFT size: one time-alignment launch per size
  std::vector<uint32_t> order_idx;
  uint32_t              group_begin[NOF_IDFT_SIZES + 1] = {};
  order_idx.reserve(nof_pdus);
  for (uint32_t s = 0; s != NOF_IDFT_SIZES; ++s) {
    group_begin[s] = static_cast<uint32_t>(order_idx.size());
    for (uint32_t i = 0; i != nof_pdus; ++i) {
      if (geo[i].info[0].idft_size == IDFT_SIZES[s]) {
        order_idx.push_back(i);
      }
    }
  }
  group_begin[NOF_IDFT_SIZES] = static_cast<uint32_t>(order_idx.size());

  hipStream_t                 s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(est->mtx);
  hipError_t                  e = hipSetDevice(est->device);
  if (e != hipSuccess) {
    return hip_fail(e, "SRS estimator device");
  }
  const size_t bytes = static_cast<size_t>(nof_pdus) * sizeof(srs_pdu);
  e                  = est->partials.ensure(static_cast<size_t>(nof_pdus) * sizeof(srs_partial));
  if (e != hipSuccess) {
    return hip_fail(e, "SRS estimator scratch");
  }
  std::vector<srs_pdu> pdus(nof_pdus);
  for (uint32_t j = 0; j != nof_pdus; ++j) {
    const uint32_t            i = order_idx[j];
    const srs_amd_srs_config& c = configs[i];
    const derived&            g = geo[i];
    srs_pdu&                  o = pdus[j];
    std::memset(&o, 0, sizeof(o));
    o.grid     = c.d_grid != nullptr ? c.d_grid : d_grids + c.grid * grid_stride;
    o.out      = d_results + i;
    o.partial  = est->partials.as<srs_partial>() + j;
    const int rc = est->sequence(g.info[0].sequence_length, g.info[0].sequence_group, o.sequence);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    o.twiddles       = est->d_twiddles[size_slot(g.info[0].idft_size)];
    o.tables         = est->d_tables;
    o.nof_subc       = nof_subc;
    o.M              = g.info[0].sequence_length;
    o.comb           = c.comb_size;
    o.nof_ap         = c.nof_antenna_ports;
    o.nof_symbols    = c.nof_symbols;
    o.start_symbol   = c.start_symbol;
    o.nof_rx         = c.nof_rx_ports;
    o.interleaved    = c.nof_antenna_ports == 4 && g.info[0].n_cs >= g.info[0].n_cs_max / 2;
    o.max_ta_samples = g.max_ta_samples;
    o.scs_khz        = g.scs_khz;
    for (uint32_t p = 0; p != c.nof_antenna_ports; ++p) {
      o.k0[p]      = g.info[p].mapping_initial_subcarrier;
      o.cs_step[p] = g.info[p].n_cs * SRS_CS_TABLE_SIZE / g.info[p].n_cs_max;
    }
    for (uint32_t r = 0; r != c.nof_rx_ports; ++r) {
      o.rx_ports[r] = c.rx_ports[r];
    }
    o.sampling_rate   = g.sampling_rate;
    o.ta_resolution_s = 1.0 / g.sampling_rate;
    o.ta_max_s        = static_cast<double>(g.max_ta_samples) / g.sampling_rate;
  }
  staged_call call("SRS estimator", staged_call::DEVICE_IS_CURRENT, est->descriptors, bytes, est->stage, bytes,
                   est->order, s);
  if (!call.ok()) {
    return call.finish();
  }
  std::memcpy(call.host(), pdus.data(), bytes);
  e                    = call.upload(est->descriptors.ptr, bytes);
  const srs_pdu* d_pdu = est->descriptors.as<srs_pdu>();
  for (uint32_t k = 0; k != NOF_IDFT_SIZES && e == hipSuccess; ++k) {
    e = launch_srs_ta(d_pdu + group_begin[k], group_begin[k + 1] - group_begin[k], IDFT_SIZES[k], s);
  }
  if (e == hipSuccess) {
    e = launch_srs_estimate(d_pdu, nof_pdus, s);
  }
  if (e == hipSuccess) {
    e = launch_srs_finish(d_pdu, nof_pdus, s);
  }
  return call.finish(e);
}

int srs_amd_srs_estimate(srs_amd_srs_estimator*    est,
                         const srs_amd_srs_config* config,
                         const uint32_t*           grid,
                         uint32_t                  nof_ports,
                         uint32_t                  nof_subc,
                         srs_amd_srs_result*       result)
{
  if (est == nullptr || config == nullptr || grid == nullptr || result == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  int     rc = derive(*config, nof_ports, nof_subc, d);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  const size_t in_bytes = static_cast<size_t>(nof_ports) * SRS_NSYMB * nof_subc * sizeof(uint32_t);
  const size_t res_off  = align_up(in_bytes, 16);
  host_call    call("SRS estimator", est->host_mtx, est->device, est->stream);
  call.grow(est->host_io, res_off + sizeof(srs_amd_srs_result));
  call.in(est->host_io.ptr, grid, in_bytes);
  if (!call.ok()) {
    return call.finish();
  }
  auto*              d_res = reinterpret_cast<srs_amd_srs_result*>(est->host_io.as<uint8_t>() + res_off);
  srs_amd_srs_config c     = *config;
  c.grid                   = 0;
  c.d_grid                 = nullptr;
  rc = srs_amd_srs_estimate_batch(est, &c, 1, est->host_io.as<uint32_t>(), 0, 1, nof_ports, nof_subc, d_res, est->stream);
  if (rc == SRS_AMD_OK) {
    call.out(result, d_res, sizeof(srs_amd_srs_result));
  }
  return call.finish(rc);
}


} // extern "C"
