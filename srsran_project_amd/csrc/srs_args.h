// srs_args.h -- per-PDU descriptor of the SRS estimator kernels (srs.hip), shared with the C-ABI (srs_api.cpp),
// which validates every field before a launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "srsran_amd/srs.h"

namespace srs_amd {

constexpr uint32_t SRS_MAX_PORTS       = SRS_AMD_SRS_MAX_PORTS;
constexpr uint32_t SRS_NSYMB           = 14;
constexpr uint32_t SRS_CEXP_TABLE_SIZE = 1024; // srs_estimator_generic_impl.h:63
constexpr uint32_t SRS_CS_TABLE_SIZE   = 24;   // low_papr_sequence_generator_impl's cs_table

// What the kernels of one PDU hand to each other (device memory, one per batch position).
struct srs_partial {
  double ta[SRS_MAX_PORTS];                         // per antenna port, seconds (srs_ta_kernel)
  float2 coefficient[SRS_MAX_PORTS][SRS_MAX_PORTS]; // [rx port index][antenna port], not yet scaled (srs_estimate_kernel)
  float  noise[SRS_MAX_PORTS];                      // per rx port index: sum of |residual|^2
  float  epre[SRS_MAX_PORTS];                       // per rx port index: sum over symbols (and pilot sets) of the mean |rx|^2
};

struct srs_pdu {
  const uint32_t*     grid;     // cbf16 [nof_grid_ports][14][nof_subc], one 32-bit word per value (real part in the low half)
  srs_amd_srs_result* out;
  srs_partial*        partial;
  const float2*       sequence; // r_{u,0}(n), n < M: the estimator's cache
  const float2*       twiddles; // W_N^m of this PDU's IDFT size
  const float2*       tables;   // exp(j 2 pi k / 1024), k < 1024, then exp(j 2 pi k / 24), k < 24
  uint32_t nof_subc;
  uint32_t M;                   // sequence length
  uint32_t comb;
  uint32_t nof_ap, nof_symbols, start_symbol, nof_rx;
  uint32_t interleaved;         // four antenna ports with n_cs >= n_cs_max / 2: odd ports on the other comb tooth
  uint32_t max_ta_samples;      // estimate_ta_correlation's search range, computed in double on the host
  uint32_t scs_khz;             // 15 << numerology
  uint32_t k0[SRS_MAX_PORTS];       // initial subcarrier per antenna port
  uint32_t cs_step[SRS_MAX_PORTS];  // n_cs x 24 / n_cs_max per antenna port
  uint8_t  rx_ports[SRS_MAX_PORTS];
  double   sampling_rate;       // N x scs x comb, Hz
  double   ta_resolution_s, ta_max_s;
};

// IDFT sizes of the time-alignment stage: get_idft's pow2ceil(M x 4096 / 3300), at least 128, for M <= 1632.
#define SRS_SRS_FOR_EACH_SIZE(X) X(128) X(256) X(512) X(1024) X(2048)

// Time alignment per antenna port: one workgroup per (antenna port, PDU) of pdus[0 .. nof), all of IDFT size N.
hipError_t launch_srs_ta(const srs_pdu* pdus, uint32_t nof, uint32_t N, hipStream_t stream);
// Coefficients, residual and EPRE: one workgroup per (rx port index, PDU).
hipError_t launch_srs_estimate(const srs_pdu* pdus, uint32_t nof, hipStream_t stream);
// Noise variance, scaling, powers in dB and the fixed result fields: one thread per PDU.
hipError_t launch_srs_finish(const srs_pdu* pdus, uint32_t nof, hipStream_t stream);

} // namespace srs_amd
