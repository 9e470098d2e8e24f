// prach_args.h -- per-occasion descriptor of the PRACH detector kernels (prach.hip), shared with the C-ABI
// (prach_api.cpp), which validates every field before a launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "srsran_amd/prach.h"

namespace srs_amd {

constexpr uint32_t PRACH_MAX_PREAMBLES = SRS_AMD_PRACH_MAX_PREAMBLES;

struct prach_occasion {
  const uint32_t*       x;        // cbf16 [port][symbol][L_ra], one 32-bit word per value (real part in the low half)
  srs_amd_prach_result* out;
  const float2*         roots;    // the detector's root cache: y_u at roots + root_slot x PRACH_ROOT_STRIDE
  const float2*         twiddles; // W_N^m of this occasion's IDFT size
  uint16_t root_slot[PRACH_MAX_PREAMBLES]; // per root sequence of the occasion
  uint32_t L_ra, nof_symbols, nof_ports;
  uint32_t combine;       // symbols summed before the correlation
  uint32_t N_cs, nof_shifts, nof_sequences;
  uint32_t win_width, win_margin;
  uint32_t start, end;    // requested preamble indices [start, end)
  uint32_t delay_limit;   // a peak is accepted at delay < delay_limit (= ceil(0.8 max_delay_samples))
  float    threshold;
  float    ms_scale;      // 1 / (N L_ra)
  float    win_scale;     // N / L_ra
  float    power_norm;    // nof_ports L_ra nof_symbols (x nof_symbols when combined)
  double   sampling_rate; // N x scs, Hz
  double   time_resolution_s, time_advance_max_s;
};

constexpr uint32_t PRACH_ROOT_STRIDE = 840; // complex values per cached root (L_ra <= 839)

// IDFT sizes with a kernel: the Stockham plans (dft_engine.h) of one or more whole wavefronts whose LDS footprint
// (transform + |.|^2 + numerator + denominator) stays below 64 KiB.
#define SRS_PRACH_FOR_EACH_SIZE(X) X(256) X(512) X(1024) X(2048)

// Correlation and metric: one workgroup per (root sequence, occasion) of occ[0 .. nof), all of IDFT size N.
hipError_t launch_prach_correlate(const prach_occasion* occ, uint32_t nof, uint32_t N, hipStream_t stream);
// RSSI, the fixed result fields and the compaction of the detected preambles: one workgroup per occasion.
hipError_t launch_prach_finish(const prach_occasion* occ, uint32_t nof, hipStream_t stream);

} // namespace srs_amd
