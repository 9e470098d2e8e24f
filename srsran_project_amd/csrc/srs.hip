// srs.hip -- MI355X SRS channel estimator kernels (srs_estimator_generic_impl.cpp:79-283,
// time_alignment_estimator_dft_impl.cpp:174-303).
//
// srs_ta_kernel<N>: one workgroup of plan<N>::T threads per (SRS antenna port, PDU).  For every receive port it runs
// one zero-padded N-point inverse DFT (dft_engine.h) whose loader forms the least-squares estimate straight from the
// cbf16 grid -- the sum over the SRS symbols of the REs at k0 + comb n, times the conjugate pilot, times
// 1 / nof_symbols -- so the padded vector never exists in memory, and whose storer accumulates |.|^2 into LDS.  An
// output sample belongs to one thread for the whole kernel, so the accumulation order over the receive ports is fixed.
// The peak rule of estimate_ta_correlation follows: the first maximum of the delayed range and of the advanced
// range, the delayed one on a tie, and the 5- or 3-tap quadratic refinement.
//
// srs_estimate_kernel: one workgroup per (receive port index, PDU).  The least-squares estimate is formed again from
// the grid (its rows are L2-resident; the tensor of a 4 x 4 x 1632 PDU would not fit LDS), compensated with the
// reference's 1024-entry exponential table at its rounded index and averaged into the wideband coefficient of every
// antenna port; a second pass over the grid removes the reconstructed pilots and sums the residual and the EPRE.
// Every sum over the sequence is a per-thread strided sum, a wavefront butterfly and an ordered sum over the
// wavefronts: no atomics, one fixed order.
//
// srs_finish_kernel: one thread per PDU -- noise variance with the reference's degrees of freedom, the clamp of the
// noise standard deviation, the scaled matrix, EPRE and RSRP in dB and the time-alignment fields.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dft_engine.h"
#include "srs_args.h"

namespace srs_amd {

namespace {

using dft::cf;

constexpr float SRS_TWOPI = 2.0F * static_cast<float>(3.14159265358979323846); // math_utils.h:36
constexpr int   EST_T     = 256;

__device__ __forceinline__ cf from_cbf16(uint32_t u)
{
  return cf{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
}

// r_{u,v}^{alpha}(n): the base sequence times the cyclic-shift table at (n step) mod 24
// (low_papr_sequence_generator_impl.cpp:263-273); no product for a zero cyclic shift.
__device__ __forceinline__ cf pilot(const float2* sequence, const float2* cs_table, uint32_t step, uint32_t n)
{
  const float2 r = sequence[n];
  if (step == 0) {
    return cf{r.x, r.y};
  }
  const float2 c = cs_table[(n * step) % SRS_CS_TABLE_SIZE];
  return dft::cmul(cf{r.x, r.y}, cf{c.x, c.y});
}

// sum over the SRS symbols of the RE of sequence element n
__device__ __forceinline__ cf rx_sum(const uint32_t* row, uint32_t nof_subc, uint32_t nof_symbols, uint32_t k)
{
  cf a = from_cbf16(row[k]);
  for (uint32_t s = 1; s < nof_symbols; ++s) {
    a = a + from_cbf16(row[static_cast<size_t>(s) * nof_subc + k]);
  }
  return a;
}

__device__ __forceinline__ float wave_sum(float v)
{
  for (int o = 32; o > 0; o >>= 1) {
    v += __shfl_xor(v, o);
  }
  return v;
}

// Sum of v over the EST_T threads of the workgroup, the same value in every thread: wavefront butterflies, then the
// wavefronts in order.  Every thread calls it; scratch holds one float per wavefront.
__device__ __forceinline__ float block_sum(float v, float* scratch)
{
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) {
    scratch[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  float s = scratch[0];
  for (int w = 1; w < EST_T / 64; ++w) {
    s += scratch[w];
  }
  __syncthreads();
  return s;
}

// compensate_phase_shift's table entry for element n (srs_estimator_generic_impl.cpp:56-77): the products and the
// sum are rounded one by one, as the expression is written.
__device__ __forceinline__ cf phase_entry(const float2* cexp_table, float phase_shift_subcarrier, float phase_shift_offset, uint32_t n)
{
  const float arg = __fadd_rn(__fmul_rn(static_cast<float>(n), phase_shift_subcarrier), phase_shift_offset);
  const int   idx = static_cast<int>(roundf(__fdiv_rn(__fmul_rn(static_cast<float>(SRS_CEXP_TABLE_SIZE), arg), SRS_TWOPI)));
  const float2 e  = cexp_table[static_cast<uint32_t>(idx) % SRS_CEXP_TABLE_SIZE];
  return cf{e.x, e.y};
}

} // namespace

template <int N>
__global__ __launch_bounds__(dft::plan<N>::T) void srs_ta_kernel(const srs_pdu* pdus)
{
  constexpr int  T  = dft::plan<N>::T;
  const srs_pdu& d  = pdus[blockIdx.y];
  const uint32_t ap = blockIdx.x;
  if (ap >= d.nof_ap) { // whole workgroup
    return;
  }
  __shared__ cf    lds[dft::lds_complex<N>()];
  __shared__ float corr[N]; // sum over the receive ports of |IDFT|^2
  __shared__ float best_v[2][T];
  __shared__ int   best_i[2][T];
  const int       tid  = threadIdx.x;
  const uint32_t  M    = d.M, comb = d.comb, nsym = d.nof_symbols, step = d.cs_step[ap];
  const float     inv  = 1.0f / static_cast<float>(nsym);
  const float2*   cs   = d.tables + SRS_CEXP_TABLE_SIZE;

  for (uint32_t r = 0; r < d.nof_rx; ++r) {
    const uint32_t* row  = d.grid + (static_cast<size_t>(d.rx_ports[r]) * SRS_NSYMB + d.start_symbol) * d.nof_subc + d.k0[ap];
    auto            load = [&](int i) -> cf {
      if (static_cast<uint32_t>(i) >= M) {
        return cf{0.0f, 0.0f};
      }
      const cf a = rx_sum(row, d.nof_subc, nsym, comb * i);
      const cf q = pilot(d.sequence, cs, step, i);
      cf       v = cf{a.x * q.x + a.y * q.y, a.y * q.x - a.x * q.y}; // a conj(q)
      if (nsym > 1) {
        v = dft::scale(v, inv);
      }
      return v;
    };
    auto store = [&](int i, cf v) {
      const float p = v.x * v.x + v.y * v.y;
      corr[i]       = r == 0 ? p : corr[i] + p;
    };
    dft::plan<N>::template engine<+1>::run(lds, reinterpret_cast<const cf*>(d.twiddles), load, store);
    __syncthreads(); // the next transform's first pass overwrites lds; the search below reads corr
  }

  // first maximum of the delayed taps [0, m) and of the advanced taps [N - m, N)
  const int m = static_cast<int>(d.max_ta_samples); // 0 < m <= N / 8
  float     vd = -1.0f, va = -1.0f;
  int       id = N, ia = N;
  for (int j = tid; j < m; j += T) {
    const float cd = corr[j], ca = corr[N - m + j];
    if (cd > vd) {
      vd = cd;
      id = j;
    }
    if (ca > va) {
      va = ca;
      ia = j;
    }
  }
  best_v[0][tid] = vd;
  best_i[0][tid] = id;
  best_v[1][tid] = va;
  best_i[1][tid] = ia;
  for (int o = T / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      for (int w = 0; w < 2; ++w) {
        const float ov = best_v[w][tid + o];
        const int   oi = best_i[w][tid + o];
        if (ov > best_v[w][tid] || (ov == best_v[w][tid] && oi < best_i[w][tid])) {
          best_v[w][tid] = ov;
          best_i[w][tid] = oi;
        }
      }
    }
  }
  if (tid == 0) {
    vd = best_v[0][0];
    va = best_v[1][0];
    id = best_i[0][0] < m ? best_i[0][0] : 0; // nothing comparable (NaN everywhere): the first tap
    ia = best_i[1][0] < m ? best_i[1][0] : 0;
    const int idx  = vd >= va ? id : -(m - ia);
    const int taps = m > 2 ? 5 : 3;
    float     pk[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      pk[i] = i < taps ? corr[static_cast<uint32_t>(idx + i + N - taps / 2) % static_cast<uint32_t>(N)] : 0.0f;
    }
    float f;
    if (taps == 5) {
      const float num = -0.4f * pk[0] + -0.2f * pk[1] + 0.0f * pk[2] + 0.2f * pk[3] + 0.4f * pk[4];
      const float den = 0.571429f * pk[0] + -0.285714f * pk[1] + -0.571429f * pk[2] + -0.285714f * pk[3] + 0.571429f * pk[4];
      f               = -1.0f * num / den;
    } else {
      const float num = -0.5f * pk[0] + 0.0f * pk[1] + 0.5f * pk[2];
      const float den = 0.5f * pk[0] + -1.0f * pk[1] + 0.5f * pk[2];
      f               = -0.5f * num / den;
    }
    const double frac = (isnan(f) || isinf(f) || fabsf(f) > 1.0f) ? 0.0 : static_cast<double>(f);
    d.partial->ta[ap] = (static_cast<double>(idx) + frac) / d.sampling_rate;
  }
}

__global__ __launch_bounds__(EST_T) void srs_estimate_kernel(const srs_pdu* pdus)
{
  const srs_pdu& d = pdus[blockIdx.y];
  const uint32_t r = blockIdx.x;
  if (r >= d.nof_rx) { // whole workgroup
    return;
  }
  __shared__ float scratch[EST_T / 64];
  const uint32_t tid  = threadIdx.x;
  const uint32_t M    = d.M, comb = d.comb, nsym = d.nof_symbols, nof_ap = d.nof_ap;
  const float2*  cexp = d.tables;
  const float2*  cs   = d.tables + SRS_CEXP_TABLE_SIZE;
  const float    inv  = 1.0f / static_cast<float>(nsym);

  // mean time alignment over the antenna ports (:200, :207)
  double ta = 0.0;
  for (uint32_t p = 0; p < nof_ap; ++p) {
    ta += d.partial->ta[p];
  }
  ta /= static_cast<double>(nof_ap);
  // phase shift per sequence element (:221-222)
  const float phase_sub = static_cast<float>(static_cast<double>(SRS_TWOPI) * ta * static_cast<double>(d.scs_khz) * 1000.0 *
                                             static_cast<double>(comb));

  const uint32_t* base = d.grid + (static_cast<size_t>(d.rx_ports[r]) * SRS_NSYMB + d.start_symbol) * d.nof_subc;

  // wideband coefficient per antenna port: the mean of the compensated least-squares estimate (:229-233)
  cf coef[SRS_MAX_PORTS];
#pragma unroll
  for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
    coef[p] = cf{0.0f, 0.0f};
    if (p < nof_ap) { // uniform
      const uint32_t* row       = base + d.k0[p];
      const float     phase_off = __fdiv_rn(__fmul_rn(phase_sub, static_cast<float>(d.k0[p])), static_cast<float>(comb));
      cf              acc       = cf{0.0f, 0.0f};
      for (uint32_t n = tid; n < M; n += EST_T) {
        const cf a = rx_sum(row, d.nof_subc, nsym, comb * n);
        const cf q = pilot(d.sequence, cs, d.cs_step[p], n);
        cf       v = cf{a.x * q.x + a.y * q.y, a.y * q.x - a.x * q.y};
        if (nsym > 1) {
          v = dft::scale(v, inv);
        }
        acc = acc + dft::cmul(v, phase_entry(cexp, phase_sub, phase_off, n));
      }
      const float re = block_sum(acc.x, scratch), im = block_sum(acc.y, scratch);
      coef[p]        = cf{re / static_cast<float>(M), im / static_cast<float>(M)};
    }
  }

  // residual: the received pilots of each pilot set, compensated, minus the reconstruction of the set's antenna
  // ports (:236-257), and the EPRE of the same REs (:169-172)
  const uint32_t nof_sets = d.interleaved ? 2 : 1;
  float          noise = 0.0f, epre = 0.0f;
  for (uint32_t set = 0; set < nof_sets; ++set) {
    const uint32_t* row       = base + d.k0[set];
    const float     phase_off = __fdiv_rn(__fmul_rn(phase_sub, static_cast<float>(d.k0[set])), static_cast<float>(comb));
    for (uint32_t n = tid; n < M; n += EST_T) {
      cf a = from_cbf16(row[comb * n]);
      epre += a.x * a.x + a.y * a.y;
      for (uint32_t s = 1; s < nsym; ++s) {
        const cf b = from_cbf16(row[static_cast<size_t>(s) * d.nof_subc + comb * n]);
        epre += b.x * b.x + b.y * b.y;
        a = a + b;
      }
      cf res = dft::cmul(a, phase_entry(cexp, phase_sub, phase_off, n));
#pragma unroll
      for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
        if (p < nof_ap && (!d.interleaved || (p & 1) == set)) {
          const cf scaled = dft::scale(coef[p], static_cast<float>(nsym));
          res             = res - dft::cmul(pilot(d.sequence, cs, d.cs_step[p], n), scaled);
        }
      }
      noise += res.x * res.x + res.y * res.y;
    }
  }
  noise = block_sum(noise, scratch);
  epre  = block_sum(epre, scratch);
  if (tid == 0) {
    srs_partial* out = d.partial;
#pragma unroll
    for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
      out->coefficient[r][p] = make_float2(coef[p].x, coef[p].y);
    }
    out->noise[r] = noise;
    out->epre[r]  = epre / static_cast<float>(M);
  }
}

__global__ __launch_bounds__(64) void srs_finish_kernel(const srs_pdu* pdus, uint32_t nof)
{
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nof) {
    return;
  }
  const srs_pdu&      d   = pdus[i];
  const srs_partial*  in  = d.partial;
  srs_amd_srs_result* out = d.out;
  float               rsrp = 0.0f, noise_var = 0.0f, epre = 0.0f;
  double              ta = 0.0;
  for (uint32_t r = 0; r < d.nof_rx; ++r) {
    for (uint32_t p = 0; p < d.nof_ap; ++p) {
      const float2 c = in->coefficient[r][p];
      rsrp += c.x * c.x + c.y * c.y;
    }
    noise_var += in->noise[r];
    epre += in->epre[r];
  }
  for (uint32_t p = 0; p < d.nof_ap; ++p) {
    ta += in->ta[p];
  }
  // degrees of freedom and correction factor (:264-266), the 40 dB clamp (:271)
  const uint32_t nof_estimates = d.interleaved ? 2 : d.nof_ap;
  const uint32_t correction    = d.interleaved ? 2 : 1;
  noise_var /= static_cast<float>((d.nof_symbols * d.M - nof_estimates) * correction * d.nof_rx);
  const float a = sqrtf(noise_var), b = sqrtf(rsrp) * 0.01f;
  const float noise_std = a < b ? b : a; // std::max
  const float scaling   = 1.0f / noise_std;
  for (uint32_t r = 0; r < SRS_MAX_PORTS; ++r) {
    for (uint32_t p = 0; p < SRS_MAX_PORTS; ++p) {
      const bool   used = r < d.nof_rx && p < d.nof_ap;
      const float2 c    = used ? in->coefficient[r][p] : make_float2(0.0f, 0.0f);
      out->channel_matrix[r][p][0] = used ? c.x * scaling : 0.0f;
      out->channel_matrix[r][p][1] = used ? c.y * scaling : 0.0f;
    }
  }
  epre /= static_cast<float>(d.nof_symbols * correction * d.nof_rx);
  rsrp /= static_cast<float>(d.nof_ap * d.nof_rx);
  out->epre_db          = 10.0f * log10f(epre);
  out->rsrp_db          = 10.0f * log10f(rsrp);
  out->noise_variance   = noise_var;
  out->reserved         = 0;
  out->time_alignment_s = ta / static_cast<double>(d.nof_ap);
  out->ta_resolution_s  = d.ta_resolution_s;
  out->ta_min_s         = -d.ta_max_s;
  out->ta_max_s         = d.ta_max_s;
}

hipError_t launch_srs_ta(const srs_pdu* pdus, uint32_t nof, uint32_t N, hipStream_t stream)
{
  if (nof == 0) {
    return hipSuccess;
  }
  switch (N) {
#define SRS_CASE(NN)                                                                                                   \
  case NN:                                                                                                             \
    hipLaunchKernelGGL(srs_ta_kernel<NN>, dim3(SRS_MAX_PORTS, nof), dim3(dft::plan<NN>::T), 0, stream, pdus);          \
    break;
    SRS_SRS_FOR_EACH_SIZE(SRS_CASE)
#undef SRS_CASE
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_srs_estimate(const srs_pdu* pdus, uint32_t nof, hipStream_t stream)
{
  if (nof == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(srs_estimate_kernel, dim3(SRS_MAX_PORTS, nof), dim3(EST_T), 0, stream, pdus);
  return hipGetLastError();
}

hipError_t launch_srs_finish(const srs_pdu* pdus, uint32_t nof, hipStream_t stream)
{
  if (nof == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(srs_finish_kernel, dim3((nof + 63) / 64), dim3(64), 0, stream, pdus, nof);
  return hipGetLastError();
}

} // namespace srs_amd
