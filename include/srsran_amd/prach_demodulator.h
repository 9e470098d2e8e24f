/*
 * srsran_amd/prach_demodulator.h -- C-ABI of the MI355X batched PRACH OFDM demodulator.
 *
 * Replaces (reference interface):
 *   ofdm_prach_demodulator::demodulate(prach_buffer& buffer, span<const cf_t> input, const configuration& config)
 *       include/srsran/phy/lower/modulation/ofdm_prach_demodulator.h:79
 *   (impl lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:32-223: per time-domain occasion and PRACH symbol
 *    one DFT of srate / ra_scs points over the samples after the cyclic prefix, and per frequency-domain occasion the
 *    L_ra subcarriers from k_start of the shifted spectrum, scaled by 1 / sqrt(dft_size) and rounded to cbf16)
 * One call demodulates any number of independent windows (cells, slots), every port, time-domain and
 * frequency-domain occasion of each, long and short formats, numerologies and DFT sizes mixed.  Its output blocks are
 * the occasions srs_amd_prach_detect_batch (prach.h) reads, so baseband samples in device memory reach detected
 * preambles without leaving the device.
 *
 * DFT sizes.  dft_size = srate_hz / ra_scs must be a whole number and either
 *   - a size with a plan of the DFT engine (128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192): one
 *     transform per symbol; or
 *   - D x M with M = 1024, else 512, else 256 (the largest that divides it) and D <= 192: D interleaved M-point
 *     transforms and a direct D-term combination of the wanted subcarriers only.
 * Sampling rates are those of ofdm.h: 15 kHz times 2^a or 3 x 2^a, 1.92 to 245.76 MHz.  Resulting table (srate in
 * MHz -> dft_size; "-" is rejected with SRS_AMD_EINVAL):
 *   srate    1.25 kHz (0,1,2)   5 kHz (3)     short formats, 15 / 30 / 60 / 120 kHz
 *    1.92      1536              384          128 / -    / -    / -
 *    2.88      2304 = 9x256      -            -   / -    / -    / -
 *    3.84      3072              768          256 / 128  / -    / -
 *    5.76      4608 = 9x512      -            384 / -    / -    / -
 *    7.68      6144             1536          512 / 256  / 128  / -
 *   11.52      9216 = 9x1024    2304 = 9x256  768 / 384  / -    / -
 *   15.36     12288 = 12x1024   3072         1024 / 512  / 256  / 128
 *   23.04     18432 = 18x1024   4608 = 9x512 1536 / 768  / 384  / -
 *   30.72     24576 = 24x1024   6144         2048 / 1024 / 512  / 256
 *   46.08     36864 = 36x1024   9216 = 9x1024 3072 / 1536 / 768 / 384
 *   61.44     49152 = 48x1024  12288 = 12x1024 4096 / 2048 / 1024 / 512
 *   92.16     73728 = 72x1024  18432 = 18x1024 6144 / 3072 / 1536 / 768
 *  122.88     98304 = 96x1024  24576 = 24x1024 8192 / 4096 / 2048 / 1024
 *  184.32    147456 = 144x1024 36864 = 36x1024 12288 = 12x1024 / 6144 / 3072 / 1536
 *  245.76    196608 = 192x1024 49152 = 48x1024 16384 = 16x1024 / 8192 / 4096 / 2048
 *
 * Numerics: float32 transforms with twiddles rounded once from double (those of the combination included), the scaling
 * in float32 and one rounding to bf16, half to even, as the reference's sc_prod into cbf16_t.  The bound against the
 * exact transform is stated in DESIGN.md.
 */
#ifndef SRSRAN_AMD_PRACH_DEMODULATOR_H
#define SRSRAN_AMD_PRACH_DEMODULATOR_H

#include "srsran_amd/prach.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srs_amd_prach_demodulator srs_amd_prach_demodulator;

/* prach_constants::MAX_NOF_PRACH_TD_OCCASIONS / MAX_NOF_PRACH_FD_OCCASIONS */
#define SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS 7
#define SRS_AMD_PRACH_DEMOD_MAX_FD_OCCASIONS 8

/* One PRACH window: ofdm_prach_demodulator::configuration (ofdm_prach_demodulator.h:44) without `port` -- every port of
 * the window is demodulated in the same call. */
typedef struct {
  uint32_t numerology;          /* PUSCH subcarrier spacing index of `slot`, 0..3 */
  uint32_t subframe_slot_index; /* slot within the subframe, < 2^numerology */
  uint32_t format;              /* srs_amd_prach_format */
  uint32_t nof_td_occasions;    /* 1 for a long format, else 1..7 */
  uint32_t nof_fd_occasions;    /* 1..8 */
  uint32_t start_symbol;        /* first OFDM symbol of the first occasion within the slot, < 14 */
  uint32_t rb_offset;           /* first PUSCH resource block of frequency-domain occasion 0 */
  uint32_t nof_prb_ul_grid;     /* uplink grid size in PUSCH resource blocks */
  uint32_t nof_ports;           /* 1..255 */
} srs_amd_prach_demod_config;

/* What the demodulator derives from a sampling rate and a configuration (host only). */
typedef struct {
  uint32_t ra_scs;       /* srs_amd_prach_scs; short formats take the PUSCH spacing */
  uint32_t L_ra;
  uint32_t dft_size;     /* srate_hz / ra_scs */
  uint32_t nof_symbols;  /* PRACH symbols (DFT windows) per time-domain occasion */
  uint32_t sub_dft_size; /* M: dft_size itself when it has a plan */
  uint32_t nof_sub_dfts; /* D = dft_size / M */
  uint64_t window_samples;    /* get_prach_window_duration(format, pusch_scs, start_symbol, nof_td_occasions) */
  uint64_t min_input_samples; /* the last sample any occasion reads, plus one */
  uint64_t nof_elements;      /* cbf16 values written: nof_td x nof_fd x nof_ports x nof_symbols x L_ra */
  uint32_t sample_offset[SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS]; /* first sample (of the cyclic prefix) per td occasion */
  uint32_t cp_samples[SRS_AMD_PRACH_DEMOD_MAX_TD_OCCASIONS];    /* symbol s of the occasion starts at
                                                                   sample_offset + cp_samples + s x dft_size */
  uint32_t k_start[SRS_AMD_PRACH_DEMOD_MAX_FD_OCCASIONS];       /* first subcarrier in the PRACH grid per fd occasion */
} srs_amd_prach_demod_geometry;

/* Uploads the twiddle tables of every DFT size `srate_hz` gives (1.25 kHz, 5 kHz and the four short spacings, where
 * they divide it into a supported size), once.  SRS_AMD_EINVAL for a sampling rate outside the table above. */
int  srs_amd_prach_demodulator_create(srs_amd_prach_demodulator** dem, uint32_t srate_hz, int device);
void srs_amd_prach_demodulator_destroy(srs_amd_prach_demodulator* dem);

/* HOST only (no device needed): checks a configuration exactly as the demodulate calls do and fills the geometry.
 * SRS_AMD_EINVAL for: an unknown format; numerology > 3, subframe_slot_index >= 2^numerology or start_symbol >= 14;
 * a reserved PRACH / PUSCH spacing pair (prach_frequency_mapping_get); nof_td_occasions = 0, above 7, or not 1 for a
 * long format; nof_fd_occasions = 0 or above 8; nof_ports = 0 or above 255; dft_size <= nof_prb_ul_grid x K x 12
 * (K = PUSCH spacing / ra_scs); k_start + L_ra >= the PRACH grid size for any fd occasion; a sampling rate outside
 * the table above, one that ra_scs does not divide into a supported dft_size, or one at which an occasion does not
 * start on a whole sample.
 * Timing (ofdm_prach_demodulator_impl.cpp:88-135), in units of kappa = 64 T_c: an occasion that does not start at
 * the beginning of the slot starts 16 kappa later, and 16 kappa later again when that is past 0.5 ms (spacings up to
 * 30 kHz); a short-format occasion that covers 0 or 0.5 ms of the subframe has a cyclic prefix 16 kappa longer; the
 * A1/B1, A2/B2 and A3/B3 formats take the B cyclic prefix on the last occasion only. */
int srs_amd_prach_demod_get_geometry(uint32_t                          srate_hz,
                                     const srs_amd_prach_demod_config* config,
                                     srs_amd_prach_demod_geometry*     geometry);

/* HOST only: the element offsets of the window's nof_td x nof_fd occasions, offsets[td x nof_fd + fd] =
 * out_offset + (td x nof_fd + fd) x nof_ports x nof_symbols x L_ra -- each is one occasion of
 * srs_amd_prach_detect_batch with nof_rx_ports = nof_ports.  offsets holds nof_td_occasions x nof_fd_occasions. */
int srs_amd_prach_demod_get_detector_offsets(uint32_t                          srate_hz,
                                             const srs_amd_prach_demod_config* config,
                                             uint64_t                          out_offset,
                                             uint64_t*                         offsets);

/* HOST, synchronous: one window.  samples: complex float, port p at samples + p x port_stride (in complex samples),
 * nof_samples >= min_input_samples valid samples each, port_stride >= nof_samples; out: nof_elements cbf16 (bf16 real,
 * bf16 imaginary) [td occasion][fd occasion][port][symbol][L_ra]. */
int srs_amd_prach_demodulate(srs_amd_prach_demodulator*        dem,
                             const srs_amd_prach_demod_config* config,
                             const float*                      samples,
                             uint64_t                          nof_samples,
                             uint64_t                          port_stride,
                             void*                             out);

/* DEVICE, asynchronous on `stream`, no host synchronisation: nof_windows windows.  Window i's port p starts
 * sample_offsets[i] + p x port_strides[i] complex samples into d_samples and holds nof_samples[i] samples; its cbf16
 * output, laid out as above, starts out_offsets[i] elements into d_out (any element alignment).  The four arrays are
 * host arrays.  Everything is validated before the first launch (additionally nof_samples[i] >= min_input_samples and
 * port_strides[i] >= nof_samples[i]); an invalid call returns SRS_AMD_EINVAL and launches nothing.
 * Launches per call: one per planned dft_size present, one per sub-transform size M (1024, 512, 256) present among
 * the windows that need the split, and, when there are such windows, one finishing launch that sums their partial
 * combinations; at most 12 + 3 + 1, four for a batch of 1.25 kHz, 5 kHz and 30 kHz windows at 30.72 MHz.  The
 * partial sums live in scratch owned by the object; a call that needs more of it than any before allocates it, which
 * waits for the device once. */
int srs_amd_prach_demodulate_batch(srs_amd_prach_demodulator*        dem,
                                   const srs_amd_prach_demod_config* configs,
                                   uint32_t                          nof_windows,
                                   const void*                       d_samples,
                                   const uint64_t*                   sample_offsets,
                                   const uint64_t*                   port_strides,
                                   const uint64_t*                   nof_samples,
                                   void*                             d_out,
                                   const uint64_t*                   out_offsets,
                                   void*                             stream);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_PRACH_DEMODULATOR_H */
