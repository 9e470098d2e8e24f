// prach_demod_args.h -- descriptors of the PRACH demodulator kernels (prach_demod.hip), shared with the C-ABI
// (prach_demod_api.cpp), which validates every field before a launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "srsran_amd/prach_demodulator.h"

namespace srs_amd {

constexpr uint32_t PRACH_DEMOD_MAX_TD = SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS;

// One window.
struct prach_demod_window {
  const float2* in;          // port 0, sample 0 of the window
  uint32_t*     out;         // cbf16 [td][fd][port][symbol][L_ra], one 32-bit word per value
  const float2* twiddles;    // W_M^m, m < M, of the (sub-)transform
  const float2* twiddles_n;  // split only: W_N^m, m < N, of the combination
  float2*       partial;     // split only: [port][td][symbol][group][fd x L_ra] partial combinations
  uint64_t      port_stride; // complex samples
  uint32_t      N, M, D;     // dft_size = D x M (D = 1: planned size)
  uint32_t      A;           // split only: adjacent residues (sub-transforms) per workgroup, D = A x nof_groups
  uint32_t      nof_ports, nof_td, nof_fd, nof_symbols, L_ra;
  uint32_t      k0, k_step;  // k_start of fd occasion f = k0 + f x k_step (k_step >= L_ra)
  uint32_t      half;        // half the PRACH grid: grid subcarrier g is DFT bin g - half (mod N)
  float         scale;       // 1 / sqrt(N)
  uint32_t      first[PRACH_DEMOD_MAX_TD]; // per td occasion: sample_offset + cp_samples
};

// One workgroup: which symbol of which window (and, split path, which group of residues).
struct prach_demod_item {
  uint32_t window; // index into the call's windows
  uint8_t  port, td, symbol, group;
};

constexpr uint32_t PRACH_DEMOD_MAX_A      = 12; // wavefronts of a split-path workgroup
constexpr uint32_t PRACH_DEMOD_FINISH_T   = 256;
constexpr uint32_t PRACH_DEMOD_ROW_SPARE  = 8;  // complex values between the rows of a split workgroup's LDS

// Sub-transform sizes of the split path: one wavefront per transform, first pass fed from registers.
#define SRS_PRACH_DEMOD_FOR_EACH_SUB(X) X(1024) X(512) X(256)

// true for a dft_size the one-transform kernel handles (a plan of dft_engine.h)
bool prach_demod_planned(uint32_t N);

// One workgroup per item, every item's window of dft_size N (planned).
hipError_t launch_prach_demod_planned(const prach_demod_window* windows,
                                      const prach_demod_item*   items,
                                      uint32_t                  nof_items,
                                      uint32_t                  N,
                                      hipStream_t               stream);
// One workgroup of PRACH_DEMOD_MAX_A wavefronts per item (a group of A adjacent residues), every item's window of
// sub-transform size M.
hipError_t launch_prach_demod_split(const prach_demod_window* windows,
                                    const prach_demod_item*   items,
                                    uint32_t                  nof_items,
                                    uint32_t                  M,
                                    hipStream_t               stream);
// One workgroup per item (group ignored): the sum over the groups, scaled and rounded.
hipError_t launch_prach_demod_finish(const prach_demod_window* windows,
                                     const prach_demod_item*   items,
                                     uint32_t                  nof_items,
                                     hipStream_t               stream);

} // namespace srs_amd
