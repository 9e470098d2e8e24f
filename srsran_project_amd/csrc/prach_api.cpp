// prach_api.cpp -- C-ABI of the MI355X PRACH detector (include/srsran_amd/prach.h): the geometry of
// prach_detector_generic_impl::detect (prach_detector_generic_impl.cpp:88-163), the frequency-domain root sequences
// (TS 38.211 Section 6.3.3.1) and the launch sequence of prach.hip.
#include "srsran_amd/prach.h"
#include "srsran_amd/ldpc.h"

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "device_buffer.h"
#include "dft_engine.h"
#include "prach_args.h"
#include "staged_call.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

using namespace srs_amd;

namespace {

#include "prach_tables.inc"

constexpr uint32_t L_LONG = 839, L_SHORT = 139;
constexpr uint32_t NOF_ROOT_SLOTS = (L_LONG - 1) + (L_SHORT - 1);
constexpr double   T_C            = 1.0 / (480000.0 * 4096.0); // TS 38.211 Section 4.1
constexpr uint32_t KAPPA          = 64;

constexpr uint32_t IDFT_SIZES[] = {
#define SRS_SIZE(NN) NN,
    SRS_PRACH_FOR_EACH_SIZE(SRS_SIZE)
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

uint32_t scs_hz(uint32_t ra_scs)
{
  switch (ra_scs) {
    case SRS_AMD_PRACH_SCS_1_25KHZ:
      return 1250;
    case SRS_AMD_PRACH_SCS_5KHZ:
      return 5000;
    default:
      return 15000u << ra_scs;
  }
}

// phy_time_unit::from_seconds(s).to_seconds() (phy_time_unit.h:275-283)
double quantize_time(double seconds)
{
  const long long t10 = static_cast<long long>(seconds / T_C * 10.0);
  return static_cast<double>(t10 / 10 + (t10 % 10) / 5) * T_C;
}

uint32_t physical_root(uint32_t L_ra, uint32_t logical)
{
  if (L_ra == L_LONG) {
    const uint32_t i = logical % (L_LONG - 1);
    const uint32_t u = PRACH_ROOT_ORDER_LONG_EVEN[i / 2];
    return (i & 1) ? L_LONG - u : u;
  }
  if (L_ra == L_SHORT) {
    const uint32_t i = logical % (L_SHORT - 1);
    const uint32_t u = i / 2 + 1;
    return (i & 1) ? L_SHORT - u : u;
  }
  return 0;
}

// What the kernels need beyond the public geometry.
struct derived {
  srs_amd_prach_geometry g;
  uint32_t               scs_hz;
  uint32_t               delay_limit;
};

int derive(const srs_amd_prach_config& c, derived& d)
{
  if (c.format > SRS_AMD_PRACH_FORMAT_A3_B3) {
    return fail(SRS_AMD_EINVAL, "Invalid PRACH format (i.e., %u).", c.format);
  }
  const prach_format_row& f = PRACH_FORMATS[c.format];
  const bool scs_ok = f.scs_class == 0   ? c.ra_scs == SRS_AMD_PRACH_SCS_1_25KHZ
                      : f.scs_class == 1 ? c.ra_scs == SRS_AMD_PRACH_SCS_5KHZ
                                         : c.ra_scs <= SRS_AMD_PRACH_SCS_120KHZ;
  if (!scs_ok) {
    return fail(SRS_AMD_EINVAL, "The RA subcarrier spacing (i.e., %u) does not fit PRACH format %u.", c.ra_scs, c.format);
  }
  if (c.restricted_set != 0) {
    return fail(SRS_AMD_EINVAL, "Unrestricted sets are not implemented.");
  }
  if (c.zero_correlation_zone >= 16) {
    return fail(SRS_AMD_EINVAL, "Reserved cyclic shift.");
  }
  if (c.root_sequence_index >= f.L_ra - 1u) {
    return fail(SRS_AMD_EINVAL, "The root sequence index (i.e., %u) exceeds the %u logical roots.", c.root_sequence_index,
                f.L_ra - 1u);
  }
  if (c.start_preamble_index + static_cast<uint64_t>(c.nof_preamble_indices) > PRACH_MAX_PREAMBLES) {
    return fail(SRS_AMD_EINVAL,
                "The start preamble index (i.e., %u) and the number of preambles to detect (i.e., %u), exceed the "
                "maximum of 64.",
                c.start_preamble_index, c.nof_preamble_indices);
  }
  if (c.nof_rx_ports == 0) {
    return fail(SRS_AMD_EINVAL, "The number of receive ports must not be zero.");
  }
  const uint32_t N = c.idft_size != 0 ? c.idft_size : (f.L_ra == L_LONG ? 1024u : 256u);
  if (size_slot(N) < 0 || N < f.L_ra) {
    return fail(SRS_AMD_EINVAL, "IDFT size %u has no plan or is below the sequence length %u.", N, f.L_ra);
  }
  if (!(c.threshold > 0.0f) || !std::isfinite(c.threshold) || c.win_margin == 0) {
    return fail(SRS_AMD_EINVAL, "Window margin and threshold must be greater than zero.");
  }
  srs_amd_prach_geometry& g = d.g;
  g.L_ra          = f.L_ra;
  g.N_cs          = PRACH_NCS_UNRESTRICTED[f.scs_class][c.zero_correlation_zone];
  g.nof_shifts    = 1;
  g.nof_sequences = PRACH_MAX_PREAMBLES;
  if (g.N_cs != 0) {
    g.nof_shifts    = std::min(PRACH_MAX_PREAMBLES, g.L_ra / g.N_cs);
    g.nof_sequences = (PRACH_MAX_PREAMBLES + g.nof_shifts - 1) / g.nof_shifts;
  }
  d.scs_hz = scs_hz(c.ra_scs);
  // cyclic prefix in the units of N_cs (prach_detector_generic_impl.cpp:128-132)
  const uint32_t cp_kappa    = f.scs_class == 2 ? f.cp_kappa >> c.ra_scs : f.cp_kappa;
  const double   cp_duration = static_cast<double>(static_cast<uint64_t>(cp_kappa) * KAPPA) * T_C;
  const uint32_t cp_prach    = static_cast<uint32_t>(std::floor(cp_duration * g.L_ra * d.scs_hz));
  const uint32_t win         = g.N_cs == 0 ? cp_prach : std::min(g.N_cs, cp_prach);
  const uint32_t max_delay   = g.N_cs == 0 ? cp_prach : std::min(std::max(g.N_cs, 1u) - 1u, cp_prach);
  g.win_width                = (win * N) / g.L_ra;
  g.max_delay_samples        = (max_delay * N) / g.L_ra;
  g.nof_symbols              = f.nof_symbols;
  g.idft_size                = N;
  g.nof_elements             = static_cast<uint64_t>(c.nof_rx_ports) * g.nof_symbols * g.L_ra;
  if (g.win_width == 0 || 2ull * c.win_margin + g.win_width > N) {
    return fail(SRS_AMD_EINVAL, "The window (margin %u, width %u) does not fit the IDFT size %u.", c.win_margin,
                g.win_width, N);
  }
  d.delay_limit = static_cast<uint32_t>(std::ceil(static_cast<double>(g.max_delay_samples) * 0.8));
  return SRS_AMD_OK;
}

// y_u[k] = sum_n x_u(n) exp(-j 2 pi n k / L), x_u(n) = exp(-j pi u n (n + 1) / L) (TS 38.211 Section 6.3.3.1), by
// one direct L-point DFT in double over a table of the 2 L-th roots of unity, rounded to float; |y_u[k]| = sqrt(L).
std::vector<float2> root_frequency_domain(uint32_t L, uint32_t u)
{
  std::vector<double> c(2 * L), s(2 * L);
  for (uint32_t m = 0; m != 2 * L; ++m) {
    const double a = -M_PI * static_cast<double>(m) / static_cast<double>(L);
    c[m]           = std::cos(a);
    s[m]           = std::sin(a);
  }
  std::vector<uint32_t> xi(L); // x_u(n) = table[xi[n]]
  for (uint64_t n = 0; n != L; ++n) {
    xi[n] = static_cast<uint32_t>((u * n * (n + 1)) % (2 * L));
  }
  std::vector<float2> y(L);
  for (uint32_t k = 0; k != L; ++k) {
    double   re = 0.0, im = 0.0;
    uint32_t t = 0; // 2 n k mod 2 L
    for (uint32_t n = 0; n != L; ++n) {
      uint32_t m = xi[n] + t;
      m          = m >= 2 * L ? m - 2 * L : m;
      re += c[m];
      im += s[m];
      t += 2 * k;
      t = t >= 2 * L ? t - 2 * L : t;
    }
    y[k] = make_float2(static_cast<float>(re), static_cast<float>(im));
  }
  return y;
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

} // namespace

struct srs_amd_prach_detector {
  int           device = 0;
  hipStream_t   stream = nullptr; // host form
  float2*       d_roots = nullptr; // [NOF_ROOT_SLOTS][PRACH_ROOT_STRIDE]: long u - 1, then short 838 + u - 1
  float2*       d_twiddles[NOF_IDFT_SIZES] = {};
  bool          root_cached[NOF_ROOT_SLOTS] = {};
  device_buffer descriptors;
  device_buffer host_io;
  pinned_stage  stage;
  stream_order  order;
  std::mutex    mtx;
  std::mutex    host_mtx; // the host form's buffer and stream

  ~srs_amd_prach_detector()
  {
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    (void)hipFree(d_roots);
    for (float2* t : d_twiddles) {
      (void)hipFree(t);
    }
  }

  // Slot of root u in the cache, computed and uploaded (blocking copy: complete before any later launch on any
  // stream) the first time it is met.
  hipError_t root_slot(uint32_t L, uint32_t u, uint16_t& slot)
  {
    slot = static_cast<uint16_t>((L == L_LONG ? 0u : L_LONG - 1u) + u - 1u);
    if (root_cached[slot]) {
      return hipSuccess;
    }
    const std::vector<float2> y = root_frequency_domain(L, u);
    const hipError_t e = hipMemcpy(d_roots + static_cast<size_t>(slot) * PRACH_ROOT_STRIDE, y.data(),
                                   y.size() * sizeof(float2), hipMemcpyHostToDevice);
    root_cached[slot]  = e == hipSuccess;
    return e;
  }
};

extern "C" {

int srs_amd_prach_get_geometry(const srs_amd_prach_config* config, srs_amd_prach_geometry* geometry)
{
  if (config == nullptr || geometry == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived   d{};
  const int rc = derive(*config, d);
  if (rc == SRS_AMD_OK) {
    *geometry = d.g;
  }
  return rc;
}

uint32_t srs_amd_prach_physical_root(uint32_t L_ra, uint32_t logical_root_index)
{
  return physical_root(L_ra, logical_root_index);
}

int srs_amd_prach_detector_create(srs_amd_prach_detector** det, int device)
{
  if (det == nullptr) {
    return fail(SRS_AMD_EINVAL, "null handle pointer");
  }
  *det   = nullptr;
  int rc = select_device(device);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  auto* d      = new srs_amd_prach_detector();
  d->device    = device;
  hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    e = hipMalloc(reinterpret_cast<void**>(&d->d_roots),
                  static_cast<size_t>(NOF_ROOT_SLOTS) * PRACH_ROOT_STRIDE * sizeof(float2));
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
    return hip_fail(e, "PRACH detector tables");
  }
  *det = d;
  return SRS_AMD_OK;
}

void srs_amd_prach_detector_destroy(srs_amd_prach_detector* det)
{
  delete det;
}

int srs_amd_prach_detect_batch(srs_amd_prach_detector*     det,
                               const srs_amd_prach_config* configs,
                               uint32_t                    nof_occasions,
                               const void*                 d_symbols,
                               const uint64_t*             offsets,
                               srs_amd_prach_result*       d_results,
                               void*                       stream)
{
  if (det == nullptr) {
    return fail(SRS_AMD_EINVAL, "null PRACH detector");
  }
  if (nof_occasions == 0) {
    return SRS_AMD_OK;
  }
  if (configs == nullptr || d_symbols == nullptr || offsets == nullptr || d_results == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  if ((reinterpret_cast<uintptr_t>(d_symbols) & 3u) != 0 || (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0) {
    return fail(SRS_AMD_EINVAL, "misaligned device buffer");
  }
  if (nof_occasions > 65535u) {
    return fail(SRS_AMD_EINVAL, "More than 65535 occasions (i.e., %u) in one batch.", nof_occasions);
  }
  // validate every occasion before anything is launched
  std::vector<derived> geo(nof_occasions);
  for (uint32_t i = 0; i != nof_occasions; ++i) {
    const int rc = derive(configs[i], geo[i]);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
  }
  // occasions grouped by IDFT size: one correlation launch per size
  std::vector<uint32_t> order_idx;
  uint32_t              group_begin[NOF_IDFT_SIZES + 1] = {};
  order_idx.reserve(nof_occasions);
  for (uint32_t s = 0; s != NOF_IDFT_SIZES; ++s) {
    group_begin[s] = static_cast<uint32_t>(order_idx.size());
    for (uint32_t i = 0; i != nof_occasions; ++i) {
      if (geo[i].g.idft_size == IDFT_SIZES[s]) {
        order_idx.push_back(i);
      }
    }
  }
  group_begin[NOF_IDFT_SIZES] = static_cast<uint32_t>(order_idx.size());

  hipStream_t                 s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(det->mtx);
  hipError_t                  e = hipSetDevice(det->device);
  const size_t                bytes = static_cast<size_t>(nof_occasions) * sizeof(prach_occasion);
  std::vector<prach_occasion> occ(nof_occasions);
  for (uint32_t j = 0; j != nof_occasions && e == hipSuccess; ++j) {
    const uint32_t                i = order_idx[j];
    const srs_amd_prach_config&   c = configs[i];
    const srs_amd_prach_geometry& g = geo[i].g;
    prach_occasion&               o = occ[j];
    std::memset(&o, 0, sizeof(o));
    o.x        = static_cast<const uint32_t*>(d_symbols) + offsets[i];
    o.out      = d_results + i;
    o.roots    = det->d_roots;
    o.twiddles = det->d_twiddles[size_slot(g.idft_size)];
    const bool     all  = c.nof_preamble_indices != 0;
    const uint32_t end  = c.start_preamble_index + c.nof_preamble_indices;
    for (uint32_t q = 0; q != g.nof_sequences && e == hipSuccess; ++q) {
      // only the roots of sequences the kernel will run (prach_detector_generic_impl.cpp:196-201)
      if (!all || q * g.nof_shifts >= end || (q + 1) * g.nof_shifts <= c.start_preamble_index) {
        continue;
      }
      e = det->root_slot(g.L_ra, physical_root(g.L_ra, c.root_sequence_index + q), o.root_slot[q]);
    }
    o.L_ra          = g.L_ra;
    o.nof_symbols   = g.nof_symbols;
    o.nof_ports     = c.nof_rx_ports;
    o.combine       = c.combine_symbols != 0;
    o.N_cs          = g.N_cs;
    o.nof_shifts    = g.nof_shifts;
    o.nof_sequences = g.nof_sequences;
    o.win_width     = g.win_width;
    o.win_margin    = c.win_margin;
    o.start         = c.start_preamble_index;
    o.end           = end;
    o.delay_limit   = geo[i].delay_limit;
    o.threshold     = c.threshold;
    o.ms_scale      = 1.0f / static_cast<float>(g.idft_size * g.L_ra);
    o.win_scale     = static_cast<float>(g.idft_size) / static_cast<float>(g.L_ra);
    o.power_norm    = static_cast<float>(c.nof_rx_ports * g.L_ra * g.nof_symbols * (o.combine ? g.nof_symbols : 1u));
    o.sampling_rate = static_cast<double>(g.idft_size * geo[i].scs_hz);
    o.time_resolution_s  = quantize_time(1.0 / o.sampling_rate);
    o.time_advance_max_s = quantize_time(static_cast<double>(g.max_delay_samples) * 0.8 / o.sampling_rate);
  }
  if (e != hipSuccess) {
    return hip_fail(e, "PRACH detector scratch");
  }
  staged_call call("PRACH detector", staged_call::DEVICE_IS_CURRENT, det->descriptors, bytes, det->stage, bytes,
                   det->order, s);
  if (!call.ok()) {
    return call.finish();
  }
  std::memcpy(call.host(), occ.data(), bytes);
  e = call.upload(det->descriptors.ptr, bytes);
  const prach_occasion* d_occ = det->descriptors.as<prach_occasion>();
  for (uint32_t k = 0; k != NOF_IDFT_SIZES && e == hipSuccess; ++k) {
    e = launch_prach_correlate(d_occ + group_begin[k], group_begin[k + 1] - group_begin[k], IDFT_SIZES[k], s);
  }
  if (e == hipSuccess) {
    e = launch_prach_finish(d_occ, nof_occasions, s);
  }
  return call.finish(e);
}

int srs_amd_prach_detect(srs_amd_prach_detector*     det,
                         const srs_amd_prach_config* config,
                         const void*                 symbols,
                         srs_amd_prach_result*       result)
{
  if (det == nullptr || config == nullptr || symbols == nullptr || result == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  derived d{};
  int     rc = derive(*config, d);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  const size_t in_bytes = d.g.nof_elements * sizeof(uint32_t);
  const size_t res_off  = align_up(in_bytes, 16);
  host_call    call("PRACH detector", det->host_mtx, det->device, det->stream);
  call.grow(det->host_io, res_off + sizeof(srs_amd_prach_result));
  call.in(det->host_io.ptr, symbols, in_bytes);
  if (!call.ok()) {
    return call.finish();
  }
  auto*          d_res  = reinterpret_cast<srs_amd_prach_result*>(det->host_io.as<uint8_t>() + res_off);
  const uint64_t offset = 0;
  rc = srs_amd_prach_detect_batch(det, config, 1, det->host_io.ptr, &offset, d_res, det->stream);
  if (rc == SRS_AMD_OK) {
    call.out(result, d_res, sizeof(srs_amd_prach_result));
  }
  return call.finish(rc);
}


} // extern "C"
