// demap_device.h -- the soft demodulation mapper of one symbol (demodulation_mapper_*.cpp, see
// modulation.hip), shared by the demapper kernels (modulation.hip) and the PUSCH equalizer that demaps and
// descrambles its own output (pusch_demod.hip), so both produce the same LLR bits from the same symbol.
// The reference's AVX2 arithmetic is reproduced without floating-point contraction by the compiler (the pragma inside
// each function keeps that independent of the including file); where the x86-64-v3 build of the reference fuses a
// product into a sum, the fused multiply-add is written out.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "modulation_args.h"

namespace srs_amd {
namespace demap {

constexpr float NEAR_ZERO = 1e-9f;

__device__ __forceinline__ float safe_rcp(float nv)
{
#pragma clang fp contract(off)
  return nv > 0.0f ? 1.0f / nv : 0.0f;
}

// median(x, lo, hi) as one v_med3_i32 (lo <= hi)
__device__ __forceinline__ int med3_int(int x, int lo, int hi)
{
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
  return r;
}

// v_cvt_i32_f32: round toward zero, out-of-range values saturate, NaN converts to 0 (the instruction's defined
// behaviour, which a C++ conversion does not promise)
__device__ __forceinline__ int cvt_i32(float x)
{
  int r;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

#ifndef DEMAP_Q_CVT
#define DEMAP_Q_CVT 1
#endif
// quantize_ps (avx2_helpers.h:121) with the scale 120 / range given: scale, clip to +-120, round half to even.
// Odd in v: the product, the rounding, the saturating conversion and the clip are all symmetric and NaN gives 0,
// so a negated scale gives the negated LLR (what descrambling by a one bit asks for).
__device__ __forceinline__ int q_simd_scaled(float v, float scale)
{
#pragma clang fp contract(off)
  const float x = v * scale;
#if DEMAP_Q_CVT
  // round, convert (NaN -> 0, infinities saturate), then clip as one v_med3_i32: the same integer as clipping the
  // float first for every x (the bounds are integers), without a per-value NaN compare and select (r06)
  return med3_int(cvt_i32(__builtin_rintf(x)), -120, 120);
#else
  // clip as one v_med3_f32 (equal to the two compares for every non-NaN x; a NaN x gives 0 below)
  const float c = __builtin_rintf(__builtin_amdgcn_fmed3f(x, -120.0f, 120.0f));
  return x != x ? 0 : static_cast<int>(c);
#endif
}

__device__ __forceinline__ int q_simd(float v, float range)
{
  return q_simd_scaled(v, 120.0f / range);
}

// scale (positive) with its sign bit set where bit k of the scrambling bits c is one: a shift and one v_bfi_b32
__device__ __forceinline__ float scrambled_scale(float scale, uint32_t c, int k)
{
  return __builtin_copysignf(scale, __uint_as_float(c << (31 - k)));
}

// log_likelihood_ratio::quantize: clip to the range, round half away from zero.
__device__ __forceinline__ int q_scalar(float v, float range)
{
#pragma clang fp contract(off)
  const float c = fabsf(v) > range ? copysignf(range, v) : v;
  return static_cast<int>(roundf(c / range * 120.0f));
}

// The interval tables of a.qm = 6 / 8 but the last have one interval count and one reciprocal width (bit for
// bit): their interval index is then computed once per component.  True for every table set the library builds
// (make_table); a set that differs keeps one index per table.  Wave-uniform: scalar compares on the arguments.
__device__ __forceinline__ bool fine_tables_share_index(const demodulate_args& a, int m)
{
  bool same = true;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    if (k < m - 1) {
      same = same && a.tab[k].n == a.tab[0].n &&
             __float_as_uint(a.tab[k].inv_width) == __float_as_uint(a.tab[0].inv_width);
    }
  }
  return same;
}

// LLRs of one symbol into o[0 .. max(qm, 1)); i: the symbol's index in its demodulation call (the
// pi/2-BPSK rotation parity), simd: the symbol lies in the reference's AVX2 blocks.
// SCR: LLR k is negated where bit k of scr is one (the symbol's Gold-sequence bits).  The 64QAM / 256QAM SIMD-block
// quantizer takes the bit as the sign of its scale factor; the other paths negate the quantized value.
// QM: the modulation where the caller knows it at compile time (1: BPSK or pi/2-BPSK by a.qm; -1: a.qm).
// lt: stage_interval_tables' LDS copy.
template <bool SCR, int QM = -1, typename T>
__device__ __forceinline__ void demap_symbol_core(const demodulate_args& a, const float* lt, float2 s, float nv,
                                                  uint32_t i, bool simd, uint32_t scr, T* o)
{
#pragma clang fp contract(off)
  const int    qm    = QM >= 2 ? QM : a.qm;
  const float  xs[2] = {s.x, s.y};
  constexpr float SQRT2 = 1.41421356237309504880f;
  // quantized LLR k, negated where its scrambling bit is one
  auto put = [&](int k, int q) { o[k] = static_cast<T>((SCR && ((scr >> k) & 1u)) ? -q : q); };
  if (QM == 1 || qm <= 1) { // BPSK / pi/2-BPSK: scalar code only
    float re = s.x, im = s.y;
    if (qm == 0 && (i & 1)) {
      const float t = re;
      re            = im;
      im            = -t;
    }
    put(0, nv > 0.0f ? q_scalar(2.0f * SQRT2 * (re + im) / nv, 24.0f) : 0);
    return;
  }
  if (qm == 2) {
    const float GAIN = 2.0f * SQRT2;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      put(c, simd ? q_simd((GAIN * xs[c]) * safe_rcp(nv), 24.0f)
                  : (nv > 0.0f ? q_scalar(GAIN * xs[c] / nv, 24.0f) : 0));
    }
    return;
  }
  if (qm == 4) {
    const float S = a.qam16_scale;
    const float G = 4.0f * S, TH = 2.0f * S;
    if (simd) {
      const float rcp = safe_rcp(nv);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float x   = xs[c];
        const float f   = G * x;
        float       l01 = fabsf(x) > TH ? (2.0f * f - copysignf(0.8f, x)) : f;
        float       l23 = 0.8f - fabsf(f);
        l01 *= rcp;
        l23 *= rcp;
        if (fabsf(x) <= NEAR_ZERO) {
          l01 = 0.0f;
          l23 = 0.0f;
        }
        put(c, q_simd(l01, 20.0f));
        put(2 + c, q_simd(l23, 20.0f));
      }
    } else {
      const bool zero = (s.x * s.x + s.y * s.y) < NEAR_ZERO;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float x = xs[c];
        if (zero || !(nv > 0.0f)) {
          put(c, 0);
          put(2 + c, 0);
          continue;
        }
        float l = G * x;
        if (fabsf(x) > TH) {
          l = __builtin_fmaf(2.0f, l, -copysignf(0.8f, x));
        }
        put(c, q_scalar(l / nv, 20.0f));
        const float l2 = __builtin_fmaf(-G, fabsf(x), 0.8f);
        put(2 + c, q_scalar(l2 / nv, 20.0f));
      }
    }
    return;
  }
  // 64QAM / 256QAM: interval functions, lt[interval][table]{slope, intercept}.  One branch per symbol around the
  // whole loop (the SIMD-block arithmetic or the scalar tail's): a branch per LLR costs its exec-mask bookkeeping
  // 2 qm times.
  const int   m   = qm / 2;
  const float rcp = safe_rcp(nv);
  if (simd) {
#if DEMAP_Q_CVT
    // |x| <= NEAR_ZERO gives LLR 0: a zero reciprocal for that component (the quantizer maps the 0 * (finite) and
    // 0 * inf = NaN products alike to 0), one select per component instead of one per LLR
    const float rc[2] = {fabsf(xs[0]) <= NEAR_ZERO ? 0.0f : rcp, fabsf(xs[1]) <= NEAR_ZERO ? 0.0f : rcp};
#else
    const float rc[2] = {rcp, rcp};
#endif
    // LLR 2 k + c from its line; the scrambling bit as the sign of the quantizer's scale 120 / 20.
    // The line is one fused multiply-add: interval_function (avx2_helpers.h:248) writes _mm256_mul_ps and
    // _mm256_add_ps, which the x86-64-v3 build of the reference contracts (as it does the scalar tail's a * b + c).
    // On a zero crossing of a line the two forms differ (0 against a residue of about 1e-8), which the reciprocal
    // of a noise variance near FLT_MIN turns into 0 against +-120 (tests/test_demapper_edges_gpu.py).
    auto emit = [&](int k, int c, float slope, float icpt) {
      float l = __builtin_fmaf(slope, xs[c], icpt) * rc[c];
#if !DEMAP_Q_CVT
      if (fabsf(xs[c]) <= NEAR_ZERO) {
        l = 0.0f;
      }
#endif
      if constexpr (SCR) {
        o[2 * k + c] = static_cast<T>(q_simd_scaled(l, scrambled_scale(120.0f / 20.0f, scr, 2 * k + c)));
      } else {
        o[2 * k + c] = static_cast<T>(q_simd(l, 20.0f));
      }
    };
    if (fine_tables_share_index(a, m)) {
      // Tables 0 .. m - 2 share the interval index, the last (LSB) table has half as many intervals of twice the
      // width and keeps a floor / convert of its own: derived from the fine index it differs where x * inv_width
      // leaves the int32 range (tools/demap_index_sweep.cpp).  Per component one 16-byte and one or two 8-byte LDS
      // reads, all issued before the first use.
      const demod_interval_table& tf = a.tab[0];
      const int                   nl = m == 4 ? a.tab[3].n : a.tab[2].n;
      const float                 wl = m == 4 ? a.tab[3].inv_width : a.tab[2].inv_width;
      float4                      f01[2];
      float2                      f2[2], fl[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float x  = xs[c];
        const int   rf = 8 * med3_int(static_cast<int>(floorf(x * tf.inv_width)) + tf.n / 2, 0, tf.n - 1);
        const int   rl = 8 * med3_int(static_cast<int>(floorf(x * wl)) + nl / 2, 0, nl - 1);
        f01[c]         = *reinterpret_cast<const float4*>(lt + rf);
        if (m == 4) {
          f2[c] = *reinterpret_cast<const float2*>(lt + rf + 4);
        }
        fl[c] = *reinterpret_cast<const float2*>(lt + rl + 2 * (m - 1));
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        emit(0, c, f01[c].x, f01[c].y);
        emit(1, c, f01[c].z, f01[c].w);
        if (m == 4) {
          emit(2, c, f2[c].x, f2[c].y);
        }
        emit(m - 1, c, fl[c].x, fl[c].y);
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { // compile-time k: the table fields are scalar loads
      if (k >= m) {
        break;
      }
      const demod_interval_table& t = a.tab[k];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int idx = med3_int(static_cast<int>(floorf(xs[c] * t.inv_width)) + t.n / 2, 0, t.n - 1);
        emit(k, c, lt[8 * idx + 2 * k], lt[8 * idx + 2 * k + 1]);
      }
    }
    return;
  }
  const bool zero = (s.x * s.x + s.y * s.y) < NEAR_ZERO;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= m) {
      break;
    }
    const demod_interval_table& t = a.tab[k];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float x = xs[c];
      int         q = 0;
      if (!zero) {
        int idx = static_cast<int>(floorf(x / t.width)) + t.n / 2;
        idx     = idx < 0 ? 0 : (idx > t.n - 1 ? t.n - 1 : idx);
        float l = __builtin_fmaf(lt[8 * idx + 2 * k], x, lt[8 * idx + 2 * k + 1]);
        l *= rcp;
        q = q_scalar(l, 20.0f);
      }
      put(2 * k + c, q);
    }
  }
}

// The plain demapper (demodulate_soft, PUCCH, the unfused PUSCH tail): int8 LLRs, no scrambling.
__device__ __forceinline__ void demap_symbol(const demodulate_args& a, const float* lt, float2 s, float nv, uint32_t i,
                                             bool simd, int8_t* o)
{
  demap_symbol_core<false>(a, lt, s, nv, i, simd, 0u, o);
}

// The demapper of a symbol of modulation QM whose LLR k is descrambled by bit k of scr; q[0 .. max(QM, 1)) in
// [-120, 120], for the caller to pack.
template <int QM>
__device__ __forceinline__ void demap_symbol_scrambled(const demodulate_args& a, const float* lt, float2 s, float nv,
                                                       uint32_t i, bool simd, uint32_t scr, int* q)
{
  demap_symbol_core<true, QM>(a, lt, s, nv, i, simd, scr, q);
}

// Floats of the interval tables' LDS copy (16-byte aligned: rows are read 16 bytes at a time).
constexpr int LT_FLOATS = 16 * 4 * 2;

// The interval tables' slopes and intercepts as [interval][table k]{slope, icpt} into LDS (32 bytes per interval):
// per-lane lookups at a data-dependent interval would otherwise be loads from the kernel-argument segment, and
// what one component needs at one interval is contiguous.
__device__ __forceinline__ void stage_interval_tables(const demodulate_args& a, float* lt)
{
  for (uint32_t x = threadIdx.x; x < LT_FLOATS; x += blockDim.x) {
    const uint32_t j = x / 8, k = (x / 2) % 4, w = x % 2;
    lt[x]            = w == 0 ? a.tab[k].slope[j] : a.tab[k].icpt[j];
  }
  __syncthreads();
}

} // namespace demap
} // namespace srs_amd
