/*
 * srsran_amd/prach.h -- C-ABI of the MI355X batched PRACH preamble detector.
 *
 * Replaces (reference interface):
 *   prach_detector::detect(const prach_buffer& input, const configuration& config)
 *       include/srsran/phy/upper/channel_processors/prach_detector.h:79
 *   (impl lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:80-356: per root sequence, the
 *    frequency-domain correlation with the root, a zero-padded inverse DFT, |.|^2, and per cyclic-shift window the
 *    ratio of the window energy to the energy around it, maximised over the delay)
 * One call detects any number of independent occasions (cells, frequency-domain occasions, slots), long and short
 * formats mixed.  Unrestricted sets only, as the reference's preamble generator.
 *
 * The detection threshold and the window margin are INPUTS: the reference takes them from a table tuned for its own
 * detector (detail::get_threshold_and_margin); an integrator supplies the values that fit the deployment.
 *
 * Numerics: float32 correlation and metric as the reference, a radix-4/16 Stockham inverse DFT instead of the
 * reference's; the window reference energy is summed in double.  Detected sets and delays equal the reference's on
 * well-separated inputs; metrics agree to the bound stated in DESIGN.md.
 */
#ifndef SRSRAN_AMD_PRACH_H
#define SRSRAN_AMD_PRACH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srs_amd_prach_detector srs_amd_prach_detector;

/* Preamble formats (TS 38.211 Tables 6.3.3.1-1 and 6.3.3.1-2), numbered as the reference's prach_format_type. */
enum srs_amd_prach_format {
  SRS_AMD_PRACH_FORMAT_0 = 0,
  SRS_AMD_PRACH_FORMAT_1,
  SRS_AMD_PRACH_FORMAT_2,
  SRS_AMD_PRACH_FORMAT_3,
  SRS_AMD_PRACH_FORMAT_A1,
  SRS_AMD_PRACH_FORMAT_A2,
  SRS_AMD_PRACH_FORMAT_A3,
  SRS_AMD_PRACH_FORMAT_B1,
  SRS_AMD_PRACH_FORMAT_B4,
  SRS_AMD_PRACH_FORMAT_C0,
  SRS_AMD_PRACH_FORMAT_C2,
  SRS_AMD_PRACH_FORMAT_A1_B1,
  SRS_AMD_PRACH_FORMAT_A2_B2,
  SRS_AMD_PRACH_FORMAT_A3_B3
};

/* Random-access subcarrier spacing, numbered as the reference's prach_subcarrier_spacing. */
enum srs_amd_prach_scs {
  SRS_AMD_PRACH_SCS_15KHZ = 0,
  SRS_AMD_PRACH_SCS_30KHZ,
  SRS_AMD_PRACH_SCS_60KHZ,
  SRS_AMD_PRACH_SCS_120KHZ,
  SRS_AMD_PRACH_SCS_1_25KHZ,
  SRS_AMD_PRACH_SCS_5KHZ
};

#define SRS_AMD_PRACH_MAX_PREAMBLES 64

/* One PRACH occasion (prach_detector::configuration plus what the reference fixes at construction). */
typedef struct {
  uint32_t format;                /* srs_amd_prach_format */
  uint32_t ra_scs;                /* srs_amd_prach_scs: 1.25 kHz for formats 0-2, 5 kHz for format 3, else 15-120 kHz */
  uint32_t root_sequence_index;   /* logical, 0..837 (long) or 0..137 (short) */
  uint32_t zero_correlation_zone; /* 0..15 */
  uint32_t restricted_set;        /* 0: unrestricted; anything else is rejected */
  uint32_t start_preamble_index;
  uint32_t nof_preamble_indices;  /* start + nof <= 64 */
  uint32_t nof_rx_ports;          /* >= 1 */
  uint32_t combine_symbols;       /* non-zero: the symbols of a port are summed before the correlation (reference default) */
  uint32_t idft_size;             /* 0: 1024 (long) / 256 (short), else 256, 512, 1024 or 2048, not below L_RA */
  float    threshold;             /* > 0 */
  uint32_t win_margin;            /* > 0, 2 win_margin + win_width <= idft_size */
} srs_amd_prach_config;

/* What the detector derives from a configuration (host only). */
typedef struct {
  uint32_t L_ra;
  uint32_t N_cs;
  uint32_t nof_shifts;    /* preambles per root sequence */
  uint32_t nof_sequences; /* root sequences of the 64 preambles */
  uint32_t win_width;     /* IDFT samples */
  uint32_t max_delay_samples;
  uint32_t nof_symbols;
  uint32_t idft_size;
  uint64_t nof_elements; /* cbf16 values of the occasion: nof_rx_ports x nof_symbols x L_ra */
} srs_amd_prach_geometry;

typedef struct {
  uint32_t preamble_index;
  int32_t  delay_samples;    /* IDFT samples */
  double   time_advance_s;   /* delay / (idft_size x scs), a whole number of T_c as phy_time_unit */
  float    detection_metric; /* peak / threshold */
  float    preamble_power_db;
} srs_amd_prach_preamble;

typedef struct {
  float   peak_over_threshold; /* NaN for an index outside the requested range (or when the RSSI is not normal) */
  int32_t delay_samples;       /* position of the peak in its window; -1 likewise */
} srs_amd_prach_window;

typedef struct {
  float    rssi_db;
  uint32_t nof_detected;
  double   time_resolution_s;
  double   time_advance_max_s;
  srs_amd_prach_preamble preambles[SRS_AMD_PRACH_MAX_PREAMBLES]; /* nof_detected entries, increasing preamble index;
                                                                    the rest zero */
  srs_amd_prach_window   windows[SRS_AMD_PRACH_MAX_PREAMBLES];   /* every preamble index (log_all_opportunities) */
} srs_amd_prach_result;

int  srs_amd_prach_detector_create(srs_amd_prach_detector** det, int device);
void srs_amd_prach_detector_destroy(srs_amd_prach_detector* det);

/* HOST only (no device needed): checks a configuration exactly as the detect calls do -- SRS_AMD_EINVAL for an
 * unknown format, a subcarrier spacing that does not fit the format, a reserved N_cs (zero_correlation_zone > 15), a
 * restricted set, a root index out of range, start + nof > 64, nof_rx_ports = 0, an IDFT size without a plan or
 * below L_RA, threshold <= 0, win_margin = 0 or 2 win_margin + win_width > idft_size -- and fills the geometry. */
int srs_amd_prach_get_geometry(const srs_amd_prach_config* config, srs_amd_prach_geometry* geometry);

/* HOST only: sequence number u of a logical root index (TS 38.211 Tables 6.3.3.1-3 / -4), L_ra 839 or 139; the index
 * wraps at 838 / 138.  0 for another L_ra. */
uint32_t srs_amd_prach_physical_root(uint32_t L_ra, uint32_t logical_root_index);

/* HOST, synchronous: one occasion.  symbols: cbf16 (bf16 real, bf16 imaginary) [port][symbol][L_ra] in host memory. */
int srs_amd_prach_detect(srs_amd_prach_detector*     det,
                         const srs_amd_prach_config* config,
                         const void*                 symbols,
                         srs_amd_prach_result*       result);

/* DEVICE, asynchronous on `stream`, no host synchronisation: nof_occasions occasions.  Occasion i's cbf16 symbols
 * [port][symbol][L_ra] start offsets[i] cbf16 elements into d_symbols (offsets: host array; any element alignment);
 * d_results[i] receives its result (device memory).  One correlation launch per IDFT size present in the batch and
 * one finishing launch.  Everything is validated before the first launch.  The first call that meets a root
 * sequence uploads its frequency-domain form with a blocking copy; the roots stay cached in the detector. */
int srs_amd_prach_detect_batch(srs_amd_prach_detector*     det,
                               const srs_amd_prach_config* configs,
                               uint32_t                    nof_occasions,
                               const void*                 d_symbols,
                               const uint64_t*             offsets,
                               srs_amd_prach_result*       d_results,
                               void*                       stream);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PRACH_H */
