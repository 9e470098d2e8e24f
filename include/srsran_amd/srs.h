/*
 * srsran_amd/srs.h -- C-ABI of the MI355X batched Sounding Reference Signal (SRS) channel estimator.
 *
 * Replaces (reference interface):
 *   srs_estimator::estimate(const resource_grid_reader& grid, const srs_estimator_configuration& config)
 *       include/srsran/phy/upper/signal_processors/srs/srs_estimator.h
 *   (impl lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:79-283 with the dependencies
 *    upper_phy_factories.cpp:630-631 gives it: low_papr_sequence_generator_impl for the pilots and
 *    time_alignment_estimator_dft_impl for the delay.  Per SRS antenna port the least-squares estimate of every
 *    receive port goes through a zero-padded inverse DFT whose summed |.|^2 gives the port's time alignment; the mean
 *    alignment is compensated, the wideband coefficient is the mean over the sequence, and the residual after
 *    removing the reconstructed pilots is the noise.)
 * One call estimates any number of independent PDUs; several may share a grid on different combs, cyclic shifts or
 * symbols.  Scope as srs_validator_generic_impl.cpp: 1, 2 or 4 antenna ports, 1..4 receive ports in any order, 1, 2 or 4
 * symbols, comb 2 or 4, no frequency hopping, no group or sequence hopping.
 *
 * Numerics: float32 as the reference, a radix-4/8/16 Stockham inverse DFT instead of the reference's, sums over the
 * sequence in a fixed tree order.  The phase compensation uses the reference's 1024-entry exponential table with its
 * rounded index, not an exact sincos.  Results agree with the reference to the bounds stated in DESIGN.md.
 *
 * One reference quirk is NOT copied: the reference's combined time_alignment.min starts at
 * numeric_limits<double>::min() (srs_estimator_generic_impl.cpp:115) -- the smallest POSITIVE double, DBL_MIN -- and
 * is then max-ed with each port's negative minimum (:201), so the reference always reports DBL_MIN.  ta_min_s here is
 * -ta_max_s, the value that line was meant to produce.
 */
#ifndef SRSRAN_AMD_SRS_H
#define SRSRAN_AMD_SRS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srs_amd_srs_estimator srs_amd_srs_estimator;

#define SRS_AMD_SRS_MAX_PORTS 4

/* One SRS PDU: srs_resource_configuration (include/srsran/ran/srs/srs_resource_configuration.h:36-156) plus the slot
 * numerology and the receive port list of srs_estimator_configuration. */
typedef struct srs_amd_srs_config {
  uint32_t nof_antenna_ports;   /* 1, 2 or 4 */
  uint32_t nof_symbols;         /* 1, 2 or 4 */
  uint32_t start_symbol;        /* start + nof_symbols <= 14 */
  uint32_t configuration_index; /* C_SRS, 0..63 */
  uint32_t sequence_id;         /* n_ID^SRS, 0..1023 */
  uint32_t bandwidth_index;     /* B_SRS, 0..3 */
  uint32_t comb_size;           /* K_TC: 2 or 4 */
  uint32_t comb_offset;         /* < comb_size */
  uint32_t cyclic_shift;        /* 0..7 (comb 2) or 0..11 (comb 4) */
  uint32_t freq_position;       /* n_RRC, 0..67 */
  uint32_t freq_shift;          /* n_shift, 0..268 */
  uint32_t freq_hopping;        /* b_hop, 0..3; must not be below bandwidth_index (no frequency hopping) */
  uint32_t hopping;             /* group or sequence hopping: must be 0 (neither) */
  uint32_t numerology;          /* 0..4: subcarrier spacing 15 kHz << numerology */
  uint32_t nof_rx_ports;        /* 1..4 */
  uint8_t  rx_ports[SRS_AMD_SRS_MAX_PORTS]; /* grid ports, any order */
  uint32_t grid;                /* index of the grid in d_grids */
  const uint32_t* d_grid;       /* non-NULL: this PDU's own DEVICE grid instead of d_grids[grid] */
} srs_amd_srs_config;

/* get_srs_information (lib/ran/srs/srs_information.cpp:38-103) of one antenna port, and the IDFT size the
 * time-alignment stage uses (time_alignment_estimator_dft_impl::get_idft, :226-243). */
typedef struct srs_amd_srs_information {
  uint32_t sequence_length;            /* M = m_SRS,b x 12 / K_TC */
  uint32_t sequence_group;             /* u */
  uint32_t sequence_number;            /* v */
  uint32_t n_cs;                       /* cyclic shift of the port */
  uint32_t n_cs_max;                   /* 8 (comb 2) or 12 (comb 4) */
  uint32_t mapping_initial_subcarrier; /* k_0 */
  uint32_t comb_size;
  uint32_t idft_size;                  /* 128, 256, 512, 1024 or 2048 */
} srs_amd_srs_information;

/* srs_estimator_result (include/srsran/phy/upper/signal_processors/srs/srs_estimator_result.h:32-48). */
typedef struct srs_amd_srs_result {
  float  channel_matrix[SRS_AMD_SRS_MAX_PORTS][SRS_AMD_SRS_MAX_PORTS][2]; /* [rx port index][antenna port][re, im],
                                            divided by the noise standard deviation; unused entries are zero */
  float  epre_db;
  float  rsrp_db;
  float  noise_variance;   /* linear */
  uint32_t reserved;
  double time_alignment_s; /* mean over the antenna ports */
  double ta_resolution_s;
  double ta_min_s;         /* -ta_max_s (the reference reports DBL_MIN, see the head of this file) */
  double ta_max_s;
} srs_amd_srs_result;

int  srs_amd_srs_estimator_create(srs_amd_srs_estimator** est, int device);
void srs_amd_srs_estimator_destroy(srs_amd_srs_estimator* est);

/* HOST only (no device needed): TS 38.211 Table 6.4.1.4.3-1, as srs_configuration_get
 * (lib/ran/srs/srs_bandwidth_configuration.cpp:63).  SRS_AMD_EINVAL for c_srs > 63 or b_srs > 3. */
int srs_amd_srs_bandwidth(uint32_t c_srs, uint32_t b_srs, uint32_t* m_srs, uint32_t* N);

/* HOST only: checks the resource part of a configuration as the estimate calls do and fills the information of
 * antenna_port (< nof_antenna_ports).  SRS_AMD_EINVAL for a port or symbol count other than 1, 2 or 4, a comb other
 * than 2 or 4, a comb offset >= the comb size, a cyclic shift > 7 with comb 2 (> 11 with comb 4), an invalid
 * (configuration_index, bandwidth_index), frequency hopping (freq_hopping < bandwidth_index), group or sequence
 * hopping, start_symbol + nof_symbols > 14, a field outside its range. */
int srs_amd_srs_get_information(const srs_amd_srs_config* config, uint32_t antenna_port, srs_amd_srs_information* info);

/* HOST only: the whole validation of the estimate calls for one PDU on grids of nof_grid_ports x 14 x nof_subc --
 * srs_amd_srs_get_information's checks plus SRS_AMD_EINVAL for an empty rx port list, more than 4 rx ports, a port
 * outside the grid, or a resource whose last RE falls outside nof_subc
 * (srs_validator_generic_impl.cpp:30-62). */
int srs_amd_srs_validate(const srs_amd_srs_config* config, uint32_t nof_grid_ports, uint32_t nof_subc);

/* HOST, synchronous: one PDU on a host grid, cbf16 (bf16 real in the low half, bf16 imaginary in the high half of a
 * 32-bit word) [nof_ports][14][nof_subc].  config->grid and config->d_grid are ignored. */
int srs_amd_srs_estimate(srs_amd_srs_estimator*    est,
                         const srs_amd_srs_config* config,
                         const uint32_t*           grid,
                         uint32_t                  nof_ports,
                         uint32_t                  nof_subc,
                         srs_amd_srs_result*       result);

/* DEVICE, asynchronous on `stream`, no host synchronisation: nof_pdus PDUs.  PDU i reads d_grids + grid x grid_stride
 * (cbf16 elements; [nof_grid_ports][14][nof_subc]) or its own d_grid of the same shape, and d_results[i] (device
 * memory) receives its result.  One time-alignment launch per IDFT size present in the batch, one estimate launch
 * and one finishing launch.  Everything is validated before the first launch.  The first call that meets a base
 * sequence (length, group) uploads it with a blocking copy; the sequences stay cached in the estimator.  A PDU's
 * result does not depend on its position in the batch, on the other PDUs or on the stream. */
int srs_amd_srs_estimate_batch(srs_amd_srs_estimator*    est,
                               const srs_amd_srs_config* configs,
                               uint32_t                  nof_pdus,
                               const uint32_t*           d_grids,
                               uint64_t                  grid_stride,
                               uint32_t                  nof_grids,
                               uint32_t                  nof_grid_ports,
                               uint32_t                  nof_subc,
                               srs_amd_srs_result*       d_results,
                               void*                     stream);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_SRS_H */
