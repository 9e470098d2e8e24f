// demap_index_sweep.cpp -- host check of the 64QAM / 256QAM soft demapper's interval indices (demap_device.h, the
// SIMD-block branch) over every float bit pattern of the symbol component x.
//
// The device computes, per table, idx = med3(cvt_i32(floor(x * inv_width)) + n / 2, 0, n - 1) with a saturating
// convert (NaN -> 0) and a 32-bit wrapping add.  All tables but the last of a QAM order share n and inv_width ("fine");
// the last ("LSB") has n / 2 intervals of twice the width.  This program compares the pair (fine index, LSB index) of
// the per-table form with candidate forms that derive the LSB index from the fine one, and with the form the kernel
// uses (one chain for the fine tables, one for the LSB table).
//
//   c++ -O2 -std=c++17 -pthread -o demap_index_sweep tools/demap_index_sweep.cpp && ./demap_index_sweep
//   (-fsanitize=address,undefined works as well: a host program with its own main)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr float NEAR_ZERO = 1e-9f;

float bits_to_float(uint32_t u)
{
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// v_cvt_i32_f32: toward zero, saturating, NaN -> 0
int32_t cvt_i32(float x)
{
  if (x != x) {
    return 0;
  }
  if (x >= 2147483648.0f) {
    return INT32_MAX;
  }
  if (x <= -2147483648.0f) {
    return INT32_MIN;
  }
  return static_cast<int32_t>(x);
}

int32_t wrap_add(int32_t a, int32_t b)
{
  return static_cast<int32_t>(static_cast<uint32_t>(a) + static_cast<uint32_t>(b));
}

int32_t med3(int32_t x, int32_t lo, int32_t hi)
{
  return x < lo ? lo : (x > hi ? hi : x);
}

// the device's index of one table
int32_t index_of(float x, float inv_width, int32_t n)
{
  volatile float p = x * inv_width; // one rounded product, as with contraction off
  return med3(wrap_add(cvt_i32(std::floor(p)), n / 2), 0, n - 1);
}

struct form_stats {
  uint64_t    bad      = 0; // patterns where the LSB index differs
  uint64_t    bad_live = 0; // ... of them with |x| > NEAR_ZERO (the LLR is not forced to 0)
  uint32_t    lo = 0, hi = 0; // smallest and largest positive differing pattern with |x| > NEAR_ZERO
  bool        any      = false;
  void note(uint32_t u, float x)
  {
    ++bad;
    if (std::fabs(x) > NEAR_ZERO || x != x) {
      ++bad_live;
      if (!any) {
        lo = hi = u;
        any     = true;
      }
      lo = u < lo ? u : lo;
      hi = u > hi ? u : hi;
    }
  }
  void merge(const form_stats& o)
  {
    bad += o.bad;
    bad_live += o.bad_live;
    if (o.any) {
      if (!any) {
        lo = o.lo;
        hi = o.hi;
        any = true;
      }
      lo = o.lo < lo ? o.lo : lo;
      hi = o.hi > hi ? o.hi : hi;
    }
  }
};

constexpr int NFORMS = 3;
const char*   FORM_NAMES[NFORMS] = {"clamped fine index >> 1", "(floor >> 1) + n/4, clamped",
                                    "own floor/convert chain (as built)"};

void sweep_range(uint64_t lo, uint64_t hi, float inv_f, int32_t n_f, float inv_l, int32_t n_l, form_stats* st,
                 uint64_t* fine_bad)
{
  for (uint64_t v = lo; v < hi; ++v) {
    const uint32_t u = static_cast<uint32_t>(v);
    const float    x = bits_to_float(u);
    // per-table form (the parent's)
    const int32_t old_f = index_of(x, inv_f, n_f);
    const int32_t old_l = index_of(x, inv_l, n_l);
    // shared fine chain
    volatile float p   = x * inv_f;
    const int32_t  F   = cvt_i32(std::floor(p));
    const int32_t  fin = med3(wrap_add(F, n_f / 2), 0, n_f - 1);
    if (fin != old_f) {
      ++*fine_bad;
    }
    const int32_t cand[NFORMS] = {fin >> 1, med3(wrap_add(F >> 1, n_f / 4), 0, n_l - 1), index_of(x, inv_l, n_l)};
    for (int f = 0; f < NFORMS; ++f) {
      if (cand[f] != old_l) {
        st[f].note(u, x);
      }
    }
  }
}

void sweep(const char* name, float a, int m)
{
  const int32_t n_f   = 1 << m, n_l = n_f / 2;
  const float   w_f   = 2.0f * a, w_l = 4.0f * a;
  const float   inv_f = 1.0f / w_f, inv_l = 1.0f / w_l;
  std::printf("%s: a = %.9g, fine n = %d inv_width = %.9g, LSB n = %d inv_width = %.9g, 2 * LSB inv_width %s fine\n",
              name, a, n_f, inv_f, n_l, inv_l, 2.0f * inv_l == inv_f ? "==" : "!=");
  const unsigned           nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<form_stats>  st(nt * NFORMS);
  std::vector<uint64_t>    fb(nt, 0);
  std::vector<std::thread> th;
  const uint64_t           total = 1ull << 32;
  for (unsigned t = 0; t < nt; ++t) {
    th.emplace_back(sweep_range, total * t / nt, total * (t + 1) / nt, inv_f, n_f, inv_l, n_l, &st[t * NFORMS], &fb[t]);
  }
  for (auto& t : th) {
    t.join();
  }
  uint64_t fine_bad = 0;
  for (unsigned t = 0; t < nt; ++t) {
    fine_bad += fb[t];
  }
  std::printf("  shared fine index differs from the per-table one at %llu of 2^32 patterns\n",
              static_cast<unsigned long long>(fine_bad));
  for (int f = 0; f < NFORMS; ++f) {
    form_stats s;
    for (unsigned t = 0; t < nt; ++t) {
      s.merge(st[t * NFORMS + f]);
    }
    std::printf("  LSB index, %-36s: %llu differ, %llu of them with |x| > 1e-9 or NaN", FORM_NAMES[f],
                static_cast<unsigned long long>(s.bad), static_cast<unsigned long long>(s.bad_live));
    if (s.any) {
      std::printf(" (patterns 0x%08x = %.9g .. 0x%08x = %.9g)", s.lo, bits_to_float(s.lo), s.hi, bits_to_float(s.hi));
    }
    std::printf("\n");
  }
}

} // namespace

int main()
{
  sweep("64QAM", 1.0f / std::sqrt(42.0f), 3);
  sweep("256QAM", 1.0f / std::sqrt(170.0f), 4);
  return 0;
}
