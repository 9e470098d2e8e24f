// prach.hip -- MI355X PRACH preamble detector kernels (prach_detector_generic_impl.cpp:80-356).
//
// prach_correlate_kernel<N>: one workgroup of plan<N>::T threads per (root sequence, occasion).  For every receive
// port (and every symbol when the symbols are not combined) it runs one zero-padded N-point inverse DFT
// (dft_engine.h) whose loader forms (sum over symbols x[k]) conj(y_u[k]) straight from the cbf16 buffer and applies
// the half-swap mapping -- the last L/2 + 1 products at the start of the vector, the first L/2 at its end -- so the
// padded vector never exists in memory, and whose storer leaves |.|^2 / (N L) in LDS.  Each cyclic-shift window then
// adds its scaled samples to the numerator and (reference energy - sample) to the denominator, both in LDS
// (nof_shifts x win_width <= N).  A window belongs to one wavefront and a window sample to one lane for the whole
// kernel, so the accumulation order over ports and symbols is fixed and needs neither atomics nor extra barriers.
// After the last port every requested window takes the first maximum of num / |den| by a wavefront reduction,
// applies the threshold and delay test and writes its dense entry and a provisional preamble entry.
//
// prach_finish_kernel: one wavefront per occasion -- RSSI, the fixed result fields, and the compaction of the
// provisional entries into increasing preamble index.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dft_engine.h"
#include "prach_args.h"

namespace srs_amd {

namespace {

using dft::cf;

constexpr double PRACH_T_C = 1.0 / (480000.0 * 4096.0); // T_c, TS 38.211 Section 4.1

__device__ __forceinline__ cf from_cbf16(uint32_t u)
{
  return cf{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}

// std::isnormal
__device__ __forceinline__ bool is_normal(float v)
{
  const float a = fabsf(v);
  return a >= 1.17549435e-38f && a < __builtin_inff();
}

// phy_time_unit::from_seconds(s).to_seconds(): the nearest whole number of T_c (phy_time_unit.h:275-283)
__device__ __forceinline__ double quantize_time(double seconds)
{
  const long long t10 = static_cast<long long>(seconds / PRACH_T_C * 10.0);
  return static_cast<double>(t10 / 10 + (t10 % 10) / 5) * PRACH_T_C;
}

__device__ __forceinline__ double wave_sum(double v)
{
  for (int o = 32; o > 0; o >>= 1) {
    v += __shfl_xor(v, o);
  }
  return v;
}

} // namespace

template <int N>
__global__ __launch_bounds__(dft::plan<N>::T) void prach_correlate_kernel(const prach_occasion* occasions)
{
  constexpr int T     = dft::plan<N>::T;
  constexpr int WAVES = T / 64;
  static_assert(T % 64 == 0, "whole wavefronts");
  const prach_occasion& o   = occasions[blockIdx.y];
  const uint32_t        seq = blockIdx.x;
  const uint32_t        nsh = o.nof_shifts, W = o.win_width, L = o.L_ra;
  const uint32_t        first = seq * nsh; // preamble index of window 0
  // sequences beyond the occasion's, or that overlap no requested preamble (whole workgroup)
  if (seq >= o.nof_sequences || o.start >= o.end || first >= o.end || first + nsh <= o.start) {
    return;
  }
  __shared__ cf    lds[dft::lds_complex<N>()];
  __shared__ float ms[N];  // |IDFT|^2 / (N L) of the current port / symbol
  __shared__ float num[N]; // [window][sample]
  __shared__ float den[N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = tid; i < nsh * W; i += T) {
    num[i] = 0.0f;
    den[i] = 0.0f;
  }
  const float2*  yu      = o.roots + static_cast<size_t>(o.root_slot[seq]) * PRACH_ROOT_STRIDE;
  const uint32_t half    = L / 2;
  const uint32_t nsum    = o.combine ? o.nof_symbols : 1;
  const uint32_t nsteps  = o.combine ? 1 : o.nof_symbols;
  const float    ms_scale = o.ms_scale, win_scale = o.win_scale;

  for (uint32_t port = 0; port < o.nof_ports; ++port) {
    for (uint32_t step = 0; step < nsteps; ++step) {
      const uint32_t* xp   = reinterpret_cast<const uint32_t*>(o.x) + (static_cast<size_t>(port) * o.nof_symbols + step) * L;
      auto            load = [&](int i) -> cf {
        uint32_t k;
        if (static_cast<uint32_t>(i) <= half) {
          k = half + i;
        } else if (static_cast<uint32_t>(i) >= N - half) {
          k = i - (N - half);
        } else {
          return cf{0.0f, 0.0f};
        }
        cf a = from_cbf16(xp[k]);
        for (uint32_t s = 1; s < nsum; ++s) {
          a = a + from_cbf16(xp[s * L + k]);
        }
        const float2 y = yu[k];
        return cf{a.x * y.x + a.y * y.y, a.y * y.x - a.x * y.y}; // a conj(y)
      };
      auto store = [&](int i, cf v) { ms[i] = (v.x * v.x + v.y * v.y) * ms_scale; };
      dft::plan<N>::template engine<+1>::run(lds, reinterpret_cast<const cf*>(o.twiddles), load, store);
      __syncthreads();
      for (uint32_t w = wave; w < nsh; w += WAVES) {
        const uint32_t ws      = (N - (o.N_cs * w * N) / L) % N;
        const uint32_t i_start = (ws + N - o.win_margin) % N;
        const uint32_t len     = 2 * o.win_margin + W; // <= N
        double         part    = 0.0;
        for (uint32_t j = lane; j < len; j += 64) {
          uint32_t idx = i_start + j;
          idx          = idx >= N ? idx - N : idx;
          part += static_cast<double>(ms[idx]);
        }
        const float reference = static_cast<float>(wave_sum(part));
        for (uint32_t j = lane; j < W; j += 64) {
          const float v    = ms[ws + j] * win_scale;
          float       diff = reference - v;
          diff             = is_normal(diff) ? diff : 1e-9f;
          num[w * W + j] += v;
          den[w * W + j] += diff;
        }
      }
      // the next transform overwrites ms only after its own barriers, which every wavefront reaches after its windows
    }
  }

  for (uint32_t w = wave; w < nsh; w += WAVES) {
    const uint32_t idx = first + w;
    if (idx < o.start || idx >= o.end) {
      continue;
    }
    float    best = -1.0f;
    uint32_t bi   = 0xffffffffu;
    for (uint32_t j = lane; j < W; j += 64) {
      const float m = num[w * W + j] / fabsf(den[w * W + j]);
      if (m > best) {
        best = m;
        bi   = j;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float    ob = __shfl_xor(best, off);
      const uint32_t oi = __shfl_xor(bi, off);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi   = oi;
      }
    }
    if (lane == 0) {
      if (bi >= W) { // no comparable metric at all
        bi   = 0;
        best = num[w * W] / fabsf(den[w * W]);
      }
      const bool             detected = best > o.threshold && bi < o.delay_limit;
      srs_amd_prach_window   win;
      srs_amd_prach_preamble p;
      win.peak_over_threshold = best / o.threshold;
      win.delay_samples       = static_cast<int32_t>(bi);
      p.preamble_index        = idx;
      p.delay_samples         = detected ? static_cast<int32_t>(bi) : -1;
      p.time_advance_s        = quantize_time(static_cast<double>(bi) / o.sampling_rate);
      p.detection_metric      = best / o.threshold;
      p.preamble_power_db     = num[w * W + bi] / o.power_norm; // linear here; prach_finish_kernel converts
      o.out->windows[idx]     = win;
      o.out->preambles[idx]   = p;
    }
  }
}

__global__ __launch_bounds__(64) void prach_finish_kernel(const prach_occasion* occasions)
{
  const prach_occasion& o    = occasions[blockIdx.x];
  const uint32_t        lane = threadIdx.x;
  const uint32_t        n    = o.nof_ports * o.nof_symbols * o.L_ra;
  const uint32_t*       x    = reinterpret_cast<const uint32_t*>(o.x);
  float                 part = 0.0f;
  for (uint32_t i = lane; i < n; i += 64) {
    const cf v = from_cbf16(x[i]);
    part += v.x * v.x + v.y * v.y;
  }
  const float rssi   = static_cast<float>(wave_sum(static_cast<double>(part)) / static_cast<double>(n));
  const bool  normal = is_normal(rssi);

  srs_amd_prach_result*  out      = o.out;
  const bool             in_range = normal && lane >= o.start && lane < o.end;
  srs_amd_prach_preamble p        = {};
  if (in_range) {
    p = out->preambles[lane];
  }
  const bool detected = in_range && p.delay_samples >= 0;
  __syncthreads(); // every provisional entry is read before any is overwritten
  const unsigned long long mask  = __ballot(detected);
  const uint32_t           count = __popcll(mask);
  if (detected) {
    p.preamble_power_db = static_cast<float>(10.0 * log10(static_cast<double>(p.preamble_power_db)));
    out->preambles[__popcll(mask & ((1ull << lane) - 1ull))] = p;
  }
  if (lane >= count) {
    out->preambles[lane] = srs_amd_prach_preamble{};
  }
  if (!in_range) {
    srs_amd_prach_window win;
    win.peak_over_threshold = __builtin_nanf("");
    win.delay_samples       = -1;
    out->windows[lane]      = win;
  }
  if (lane == 0) {
    out->rssi_db            = static_cast<float>(10.0 * log10(static_cast<double>(rssi)));
    out->nof_detected       = count;
    out->time_resolution_s  = o.time_resolution_s;
    out->time_advance_max_s = o.time_advance_max_s;
  }
}

hipError_t launch_prach_correlate(const prach_occasion* occ, uint32_t nof, uint32_t N, hipStream_t stream)
{
  if (nof == 0) {
    return hipSuccess;
  }
  switch (N) {
#define SRS_CASE(NN)                                                                                                   \
  case NN:                                                                                                             \
    hipLaunchKernelGGL(prach_correlate_kernel<NN>, dim3(PRACH_MAX_PREAMBLES, nof), dim3(dft::plan<NN>::T), 0, stream,  \
                       occ);                                                                                           \
    break;
    SRS_PRACH_FOR_EACH_SIZE(SRS_CASE)
#undef SRS_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_prach_finish(const prach_occasion* occ, uint32_t nof, hipStream_t stream)
{
  if (nof == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(prach_finish_kernel, dim3(nof), dim3(64), 0, stream, occ);
  return hipGetLastError();
}

} // namespace srs_amd
