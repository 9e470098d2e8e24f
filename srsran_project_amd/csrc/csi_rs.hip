// csi_rs.hip -- MI355X NZP-CSI-RS generator kernel.
//
// csi_rs_map_kernel does in one pass what the reference does per CDM group in four
// (nzp_csi_rs_generator_impl.cpp:216-288): the Gold sequence of the group's OFDM symbol (generate_sequence, :111-139),
// the CDM weights (apply_cdm, :291-353), the precoding (channel_precoder_avx2.cpp:77-127) and the RE mapping
// (resource_grid_mapper_impl.cpp:180-307).
// One wave per (resource, CDM group): the longest symbol sequence is 3 x 275 = 825 elements = 1,650 Gold bits = 52
// words, so lane j generates word j -- the jump to the symbol's first bit (which is not word-aligned: the skipped
// prefix is 2, 4 or 6 bits per PRB) runs once per wave on the scalar unit, the lane offset by gold_state_lanes.  The
// words are then handed round the wave (one shuffle per 64 elements) so that lane j owns elements j, j + 64, ...:
// consecutive lanes store to consecutive CSI-RS subcarriers of one grid row.  Nothing is staged in memory between the
// sequence and the grid, there are no atomics, every RE is written by exactly one lane.
//
// The kernel is launch-latency bound: a slot's resources are a few thousand REs.
#include <hip/hip_runtime.h>

#include "bf16_device.h"

#include "csi_rs_args.h"
#include "gold_sequence.h"

#pragma clang fp contract(off)

namespace srs_amd {
namespace {

constexpr int CSI_RS_WAVES   = 4;
constexpr int CSI_RS_THREADS = 64 * CSI_RS_WAVES;

// x * w as _mm256_fmaddsub_ps(x, w.re, swap(x) * w.im) (channel_precoder_avx2.cpp:55-58).
__device__ __forceinline__ float2 cmul_simd(float2 x, float wr, float wi)
{
  return make_float2(__builtin_fmaf(x.x, wr, -(x.y * wi)), __builtin_fmaf(x.y, wr, x.x * wi));
}

__global__ __launch_bounds__(CSI_RS_THREADS) void csi_rs_map_kernel(const csi_rs_item* items, uint32_t nof_items,
                                                                   const uint32_t* jump)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * CSI_RS_WAVES + (threadIdx.x >> 6));
  if (item >= nof_items) {
    return; // uniform over the wave
  }
  const csi_rs_item& a = items[item];

  // lane j: bits skip_bits + 32 j .. + 31 of the symbol's sequence, elements 16 j .. 16 j + 15
  uint32_t x1, x2;
  gold_state_lanes(jump, a.c_init, a.skip_bits, lane, x1, x2);
  const uint32_t word = gold_next32(x1, x2);

  const uint32_t seq_len = __builtin_amdgcn_readfirstlane(a.seq_len);
  const uint32_t per_prb = __builtin_amdgcn_readfirstlane(a.per_prb);
  const uint32_t nof_tx  = __builtin_amdgcn_readfirstlane(a.nof_tx);
  const bool     pair    = __builtin_amdgcn_readfirstlane(a.group_size) == 2;
  const bool     bypass  = __builtin_amdgcn_readfirstlane(a.bypass) != 0;
  const float    amp     = a.amplitude;
  uint32_t*      row     = a.grid + static_cast<uint64_t>(a.symbol) * a.nof_subc;
  const uint64_t port_stride = static_cast<uint64_t>(CSI_RS_NSYMB) * a.nof_subc;

  for (uint32_t e0 = 0; e0 < seq_len; e0 += 64) {
    // element e = e0 + lane lies in the word of lane e / 16
    const uint32_t e = e0 + lane;
    const uint32_t w = __shfl(word, static_cast<int>(e >> 4), 64);
    const uint32_t bits = w >> (2u * (e & 15u));
    const float2   x    = make_float2((bits & 1u) ? -amp : amp, (bits & 2u) ? -amp : amp);
    const uint32_t prb  = e / per_prb;
    const uint32_t r    = e - prb * per_prb;
    const uint32_t k    = a.first_subc + prb * a.prb_step + a.k_bar + r * a.k_step;
    if (e >= seq_len || k >= a.nof_subc) {
      // past the sequence (k beyond the grid is excluded by the validation)
    } else if (bypass) {
      row[k] = cbf16_pack(x.x, x.y);
    } else {
      // second port of an fd-CDM2 group: w_f(k') = -1 on the odd elements (Table 7.4.1.5.3-3)
      const float2 x_odd = (e & 1u) ? make_float2(-x.x, -x.y) : x;
#pragma unroll
      for (uint32_t p = 0; p < CSI_RS_MAX_PORTS; ++p) {
        if (p < nof_tx) {
          float2 y = cmul_simd(x, a.w[0][p][0], a.w[0][p][1]);
          if (pair) {
            const float2 t = cmul_simd(x_odd, a.w[1][p][0], a.w[1][p][1]);
            y.x            = y.x + t.x;
            y.y            = y.y + t.y;
          }
          row[p * port_stride + k] = cbf16_pack(y.x, y.y);
        }
      }
    }
  }
}

} // namespace

hipError_t launch_csi_rs_map(const csi_rs_item* items, uint32_t nof_items, const uint32_t* jump, hipStream_t stream)
{
  if (nof_items == 0) {
    return hipSuccess;
  }
  const dim3 grid((nof_items + CSI_RS_WAVES - 1) / CSI_RS_WAVES);
  hipLaunchKernelGGL(csi_rs_map_kernel, grid, dim3(CSI_RS_THREADS), 0, stream, items, nof_items, jump);
  return hipGetLastError();
}

} // namespace srs_amd
