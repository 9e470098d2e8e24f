// prach_demod.hip -- MI355X PRACH OFDM demodulator kernels (ofdm_prach_demodulator_impl.cpp:32-223).
//
// A PRACH symbol is one N-point DFT, N = srate / ra_scs, of which only the nof_fd x L_ra subcarriers of the
// frequency-domain occasions are kept: grid subcarrier g is DFT bin g - grid / 2 (mod N), scaled by 1 / sqrt(N) in
// float and rounded to cbf16.
//
// prach_demod_planned_kernel<N> (N has a plan in dft_engine.h): one workgroup per (window, port, td occasion, symbol),
// one Stockham transform whose loader streams the N samples after the cyclic prefix and whose storer writes the wanted
// bins of every fd occasion -- the symbol is transformed once however many occasions read it.
//
// N = D x M without a plan (M = 1024, 512 or 256): with n = D m + r,
//   X[k] = sum_{r < D} W_N^{r k} F_r[k mod M],   F_r = DFT_M(x[D m + r]).
// prach_demod_split_kernel<M>: one workgroup of 12 wavefronts per (symbol, group of A <= 12 adjacent residues r).  The
// workgroup reads its samples as runs of A consecutive complex values every D (whole contiguous runs, each sample
// once), separates them through LDS into one row per residue, and every wavefront transforms its row: the first pass
// takes its input from registers, the passes between exchange through the wavefront's LDS row, the last pass leaves
// F_r in registers and then in the row.  The workgroup then forms, for the wanted bins only, the partial combination
// over its A residues with W_N^{r k} read from a table of exactly rounded values, and writes it to scratch.
// prach_demod_finish_kernel: sums the D / A partial combinations of every wanted bin in a fixed order, scales, rounds
// and writes the cbf16 output.
//
// The split path moves 8 N bytes in per symbol; what it writes and reads back is (D / A) x nof_fd x L_ra x 8 bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf16_device.h"
#include "dft_engine.h"
#include "prach_demod_args.h"

namespace srs_amd {

namespace {

using dft::cf;

// the baseband samples of the planned path are read once by one workgroup: keep them out of the caches
__device__ __forceinline__ cf stream_load(const cf* p)
{
  return __builtin_bit_cast(cf, __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(p)));
}

// first output word of (td, fd 0, port, symbol) and the distance between fd occasions, in cbf16 words
__device__ __forceinline__ uint32_t* symbol_out(const prach_demod_window& w, const prach_demod_item& it)
{
  const size_t row = (static_cast<size_t>(it.td) * w.nof_fd * w.nof_ports + it.port) * w.nof_symbols + it.symbol;
  return w.out + row * w.L_ra;
}
__device__ __forceinline__ size_t fd_stride(const prach_demod_window& w)
{
  return static_cast<size_t>(w.nof_ports) * w.nof_symbols * w.L_ra;
}

// DFT bin of grid subcarrier g
__device__ __forceinline__ uint32_t bin_of(const prach_demod_window& w, uint32_t g)
{
  return g < w.half ? w.N - w.half + g : g - w.half;
}

} // namespace

template <int N>
__global__ __launch_bounds__(dft::plan<N>::T) void prach_demod_planned_kernel(const prach_demod_window* windows,
                                                                              const prach_demod_item*   items)
{
  __shared__ cf             lds[dft::lds_complex<N>()];
  const prach_demod_item    it = items[blockIdx.x];
  const prach_demod_window& w  = windows[it.window];
  const cf*      in   = reinterpret_cast<const cf*>(w.in) + it.port * w.port_stride + w.first[it.td] +
                        static_cast<size_t>(it.symbol) * N;
  uint32_t*      out  = symbol_out(w, it);
  const size_t   fds  = fd_stride(w);
  const uint32_t half = w.half, k0 = w.k0, step = w.k_step, L = w.L_ra, nof_fd = w.nof_fd;
  const float    scale = w.scale;

  auto load  = [&](int i) -> cf { return stream_load(in + i); };
  auto store = [&](int k, cf v) {
    const uint32_t uk = static_cast<uint32_t>(k);
    uint32_t       g;
    if (uk >= N - half) {
      g = uk - (N - half);
    } else if (uk < half) {
      g = uk + half;
    } else {
      return; // outside the PRACH grid
    }
    if (g < k0) {
      return;
    }
    const uint32_t d = g - k0, f = d / step, b = d - f * step;
    if (f < nof_fd && b < L) {
      out[f * fds + b] = cbf16_pack(v.x * scale, v.y * scale);
    }
  };
  dft::plan<N>::template engine<-1>::run(lds, reinterpret_cast<const cf*>(w.twiddles), load, store);
}

namespace {

// Radix sequence of the one-wavefront transforms: the first radix is M / 64, so that the first pass has one butterfly
// per lane and reads lane + 64 r, r < M / 64, from registers.
template <int M, int Ns, int R, int... Rest>
__device__ __forceinline__ void wave_pass(cf* row, const cf* tw, cf* x, int lane)
{
  constexpr int  NB    = M / R;
  constexpr int  PER   = NB / 64;
  constexpr bool FIRST = Ns == 1;
  constexpr bool LAST  = sizeof...(Rest) == 0;
  static_assert(NB % 64 == 0 && (!FIRST || (PER == 1 && R == M / 64)), "one first-pass butterfly per lane");
  cf v[PER][R];
#pragma unroll
  for (int b = 0; b < PER; ++b) {
    const int j = lane + 64 * b;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (FIRST) {
        v[b][r] = x[r];
      } else {
        v[b][r] = row[dft::pad(j + r * NB)];
      }
    }
    if constexpr (!FIRST) {
      cf w[R];
      dft::twiddle_powers<R>(tw[(j % Ns) * (M / (Ns * R))], w);
#pragma unroll
      for (int r = 1; r < R; ++r) {
        v[b][r] = dft::cmul(v[b][r], w[r]);
      }
    }
    dft::small_dft<R, -1>::run(v[b]);
  }
  if constexpr (LAST) {
    // j < Ns = NB: output j + r NB = lane + 64 (b + r PER)
#pragma unroll
    for (int b = 0; b < PER; ++b) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        x[b + r * PER] = v[b][r];
      }
    }
  } else {
    if constexpr (!FIRST) {
      __syncthreads(); // every lane has read this pass's input
    }
#pragma unroll
    for (int b = 0; b < PER; ++b) {
      const int j    = lane + 64 * b;
      const int k    = j % Ns;
      const int base = (j / Ns) * Ns * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        row[dft::pad(base + r * Ns)] = v[b][r];
      }
    }
    __syncthreads();
    wave_pass<M, Ns * R, Rest...>(row, tw, x, lane);
  }
}

template <int M>
struct wave_dft;
template <>
struct wave_dft<1024> {
  __device__ __forceinline__ static void run(cf* row, const cf* tw, cf* x, int lane) { wave_pass<1024, 1, 16, 16, 4>(row, tw, x, lane); }
};
template <>
struct wave_dft<512> {
  __device__ __forceinline__ static void run(cf* row, const cf* tw, cf* x, int lane) { wave_pass<512, 1, 8, 8, 8>(row, tw, x, lane); }
};
template <>
struct wave_dft<256> {
  __device__ __forceinline__ static void run(cf* row, const cf* tw, cf* x, int lane) { wave_pass<256, 1, 4, 4, 4, 4>(row, tw, x, lane); }
};

constexpr int SPLIT_T = static_cast<int>(PRACH_DEMOD_MAX_A) * 64;

template <int M>
constexpr int split_row()
{
  return dft::lds_complex<M>() + static_cast<int>(PRACH_DEMOD_ROW_SPARE);
}

} // namespace

template <int M>
__global__ __launch_bounds__(SPLIT_T) void prach_demod_split_kernel(const prach_demod_window* windows,
                                                                    const prach_demod_item*   items)
{
  constexpr int PER = M / 64;        // values per lane of a transform, and loads per thread of the workgroup
  constexpr int RS  = split_row<M>(); // one LDS row per residue; wavefronts beyond A work on rows nobody reads
  __shared__ cf             lds[PRACH_DEMOD_MAX_A * RS];
  const prach_demod_item    it = items[blockIdx.x];
  const prach_demod_window& w  = windows[it.window];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t A = w.A, D = w.D, N = w.N;
  const uint32_t r0 = it.group * A;
  const cf*      in = reinterpret_cast<const cf*>(w.in) + it.port * w.port_stride + w.first[it.td] +
                      static_cast<size_t>(it.symbol) * N + r0;

  // runs of A consecutive samples every D: thread e takes value e mod A of run e div A
  cf       t[PER];
  uint32_t at[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const uint32_t e = tid + static_cast<uint32_t>(j) * SPLIT_T;
    const uint32_t m = e / A, i = e - m * A;
    at[j] = m < static_cast<uint32_t>(M) ? i * RS + dft::pad(static_cast<int>(m)) : 0xffffffffu;
    t[j]  = m < static_cast<uint32_t>(M) ? in[static_cast<size_t>(m) * D + i] : cf{0.0f, 0.0f};
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (at[j] != 0xffffffffu) {
      lds[at[j]] = t[j];
    }
  }
  __syncthreads();
  cf* row = lds + wave * RS;
  cf  x[PER];
#pragma unroll
  for (int s = 0; s < PER; ++s) {
    x[s] = row[dft::pad(static_cast<int>(lane) + 64 * s)];
  }
  __syncthreads();
  wave_dft<M>::run(row, reinterpret_cast<const cf*>(w.twiddles), x, static_cast<int>(lane));
  __syncthreads(); // the last pass's reads of the row are done
#pragma unroll
  for (int s = 0; s < PER; ++s) {
    row[lane + 64 * s] = x[s]; // F_r[lane + 64 s]
  }
  __syncthreads();

  // partial combination over this group's residues, wanted bins only
  const uint32_t L = w.L_ra, FL = w.nof_fd * L, G = D / A;
  const cf*      twn = reinterpret_cast<const cf*>(w.twiddles_n);
  const size_t   sym = (static_cast<size_t>(it.port) * w.nof_td + it.td) * w.nof_symbols + it.symbol;
  cf*            part = reinterpret_cast<cf*>(w.partial) + (sym * G + it.group) * FL;
  for (uint32_t o = tid; o < FL; o += SPLIT_T) {
    const uint32_t f = o / L, b = o - f * L;
    const uint32_t k = bin_of(w, w.k0 + f * w.k_step + b);
    const uint32_t q = k & static_cast<uint32_t>(M - 1);
    uint32_t       ti = static_cast<uint32_t>((static_cast<uint64_t>(r0) * k) % N); // (r k) mod N
    // every twiddle of the output is requested before the first is used: the table reads are gathers that miss the
    // vector cache, and one after the other their latencies would add up
    cf tw[PRACH_DEMOD_MAX_A];
#pragma unroll
    for (uint32_t i = 0; i < PRACH_DEMOD_MAX_A; ++i) {
      tw[i] = i < A ? twn[ti] : cf{0.0f, 0.0f};
      ti += k;
      ti = ti >= N ? ti - N : ti;
    }
    cf acc = {0.0f, 0.0f};
#pragma unroll
    for (uint32_t i = 0; i < PRACH_DEMOD_MAX_A; ++i) {
      if (i < A) {
        acc = acc + dft::cmul(lds[i * RS + q], tw[i]);
      }
    }
    part[o] = acc;
  }
}

__global__ __launch_bounds__(PRACH_DEMOD_FINISH_T) void prach_demod_finish_kernel(const prach_demod_window* windows,
                                                                                  const prach_demod_item*   items)
{
  const prach_demod_item    it = items[blockIdx.x];
  const prach_demod_window& w  = windows[it.window];
  const uint32_t L = w.L_ra, FL = w.nof_fd * L, G = w.D / w.A;
  const size_t   sym  = (static_cast<size_t>(it.port) * w.nof_td + it.td) * w.nof_symbols + it.symbol;
  const cf*      part = reinterpret_cast<const cf*>(w.partial) + sym * G * FL;
  uint32_t*      out  = symbol_out(w, it);
  const size_t   fds  = fd_stride(w);
  const float    scale = w.scale;
  for (uint32_t o = threadIdx.x; o < FL; o += PRACH_DEMOD_FINISH_T) {
    cf acc = part[o];
    for (uint32_t g = 1; g < G; ++g) {
      acc = acc + part[static_cast<size_t>(g) * FL + o];
    }
    const uint32_t f = o / L, b = o - f * L;
    out[f * fds + b] = cbf16_pack(acc.x * scale, acc.y * scale);
  }
}

bool prach_demod_planned(uint32_t N)
{
#define SRS_CASE(NN)                                                                                                   \
  if (N == NN)                                                                                                         \
    return true;
  SRS_DFT_FOR_EACH_SIZE(SRS_CASE)
#undef SRS_CASE
  return false;
}

hipError_t launch_prach_demod_planned(const prach_demod_window* windows,
                                      const prach_demod_item*   items,
                                      uint32_t                  nof_items,
                                      uint32_t                  N,
                                      hipStream_t               stream)
{
  if (nof_items == 0) {
    return hipSuccess;
  }
#define SRS_CASE(NN)                                                                                                   \
  if (N == NN) {                                                                                                       \
    hipLaunchKernelGGL(prach_demod_planned_kernel<NN>, dim3(nof_items), dim3(dft::plan<NN>::T), 0, stream, windows,    \
                       items);                                                                                         \
    return hipGetLastError();                                                                                          \
  }
  SRS_DFT_FOR_EACH_SIZE(SRS_CASE)
#undef SRS_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_prach_demod_split(const prach_demod_window* windows,
                                    const prach_demod_item*   items,
                                    uint32_t                  nof_items,
                                    uint32_t                  M,
                                    hipStream_t               stream)
{
  if (nof_items == 0) {
    return hipSuccess;
  }
#define SRS_CASE(MM)                                                                                                   \
  if (M == MM) {                                                                                                       \
    hipLaunchKernelGGL(prach_demod_split_kernel<MM>, dim3(nof_items), dim3(SPLIT_T), 0, stream, windows, items);       \
    return hipGetLastError();                                                                                          \
  }
  SRS_PRACH_DEMOD_FOR_EACH_SUB(SRS_CASE)
#undef SRS_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_prach_demod_finish(const prach_demod_window* windows,
                                     const prach_demod_item*   items,
                                     uint32_t                  nof_items,
                                     hipStream_t               stream)
{
  if (nof_items == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(prach_demod_finish_kernel, dim3(nof_items), dim3(PRACH_DEMOD_FINISH_T), 0, stream, windows, items);
  return hipGetLastError();
}

} // namespace srs_amd
