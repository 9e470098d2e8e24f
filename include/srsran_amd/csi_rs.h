/*
 * srsran_amd/csi_rs.h -- C-ABI of the MI355X batched NZP-CSI-RS generator.
 *
 * Replaces (reference interface):
 *   nzp_csi_rs_generator::map(resource_grid_writer& grid, const config_t& config)
 *       include/srsran/phy/upper/signal_processors/nzp_csi_rs/nzp_csi_rs_generator.h:88
 *   (impl lib/phy/upper/signal_processors/nzp_csi_rs/nzp_csi_rs_generator_impl.cpp:111-353 with the pattern of
 *    get_csi_rs_pattern, lib/ran/csi_rs/csi_rs_pattern.cpp:438, and the precoding and mapping of
 *    resource_grid_mapper_impl::map(writer, re_buffer, re_pattern, precoding),
 *    lib/phy/support/resource_grid_mapper_impl.cpp:180-307.  Per CDM group and OFDM symbol the Gold sequence of
 *    TS 38.211 7.4.1.5.2 is cut to the occupied PRBs, spread with w_f(k') w_t(l') over the ports of the group,
 *    precoded onto every transmit port and written to the grid.)
 * One call maps any number of resources into any number of grids (a TRS slot: two row-1 resources per grid).
 *
 * Scope: the pattern helpers cover rows 1-12 of Table 7.4.1.5.3-1, every row the reference builds.  Mapping covers
 * rows 1-5 (1, 2 or 4 ports: precoding_constants::MAX_NOF_PORTS is 4), one precoding PRG (the reference's CDM group
 * precoding is built with a single PRG, nzp_csi_rs_generator_impl.cpp:228), normal cyclic prefix.
 *
 * Numerics: the values are the reference's bit for bit -- the same product form as its SIMD precoder
 * (x * w = fmaddsub(x, w.re, swap(x) * w.im), layers added in order) rounded to bf16 half to even; a one-port resource
 * whose weight is exactly 1.0 is rounded without a product, as the mapper's bypass does
 * (resource_grid_mapper_impl.cpp:246-256).
 */
#ifndef SRSRAN_AMD_CSI_RS_H
#define SRSRAN_AMD_CSI_RS_H

#include <stdint.h>

#include "srsran_amd/pdsch_modulator.h" /* srs_amd_re_pattern, SRS_AMD_MAX_RE_PATTERNS */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srs_amd_csi_rs_generator srs_amd_csi_rs_generator;

#define SRS_AMD_CSI_RS_MAX_K_REF 6          /* CSI_RS_MAX_NOF_K_INDEXES */
#define SRS_AMD_CSI_RS_MAX_PATTERN_PORTS 16 /* rows 11 and 12 */
#define SRS_AMD_CSI_RS_MAX_PORTS 4          /* ports a resource can be mapped with */

/* nzp_csi_rs_generator::config_t (nzp_csi_rs_generator.h:46-80). */
typedef struct srs_amd_csi_rs_config {
  uint32_t numerology;   /* 0..4 */
  uint32_t slot_index;   /* slot within the frame, < 10 << numerology */
  uint32_t start_rb;     /* CRB */
  uint32_t nof_rb;
  uint32_t row;          /* Table 7.4.1.5.3-1 */
  uint32_t nof_k_ref;
  uint32_t k_ref[SRS_AMD_CSI_RS_MAX_K_REF]; /* k_0, k_1, ... */
  uint32_t symbol_l0;
  uint32_t symbol_l1;    /* carried as the reference does; rows 1-12 do not use it */
  uint32_t cdm;          /* 0 none, 1 fd-CDM2, 2 cdm4-FD2-TD2, 3 cdm8-FD2-TD4 */
  uint32_t freq_density; /* 0 three, 1 one, 2 dot5 on even RBs, 3 dot5 on odd RBs */
  uint32_t scrambling_id; /* 0..1023 */
  float    amplitude;
  float    weights[SRS_AMD_CSI_RS_MAX_PORTS][SRS_AMD_CSI_RS_MAX_PORTS][2]; /* [CSI-RS port][tx port] (re, im), the
                            whole band; the number of tx ports is the row's port count (the reference asserts
                            ports == layers == the row's ports, nzp_csi_rs_generator_impl.cpp:179-187) */
  uint32_t  grid;        /* index of the grid in d_grids */
  uint32_t* d_grid;      /* non-NULL: this resource's own DEVICE grid instead of d_grids[grid] */
} srs_amd_csi_rs_config;

/* csi_rs_pattern (include/srsran/ran/csi_rs/csi_rs_pattern.h): PRBs rb_begin, rb_begin + rb_stride, ... < rb_end. */
typedef struct srs_amd_csi_rs_pattern_port {
  uint16_t re_mask;     /* bit k = subcarrier k of the PRB */
  uint16_t symbol_mask; /* bit l = OFDM symbol l */
} srs_amd_csi_rs_pattern_port;

typedef struct srs_amd_csi_rs_pattern_desc {
  uint32_t                    rb_begin, rb_end, rb_stride;
  uint32_t                    nof_ports;
  srs_amd_csi_rs_pattern_port port[SRS_AMD_CSI_RS_MAX_PATTERN_PORTS];
} srs_amd_csi_rs_pattern_desc;

int  srs_amd_csi_rs_generator_create(srs_amd_csi_rs_generator** gen, int device);
void srs_amd_csi_rs_generator_destroy(srs_amd_csi_rs_generator* gen);

/* HOST only (no device needed): get_csi_rs_pattern (lib/ran/csi_rs/csi_rs_pattern.cpp:438) for rows 1-12, whatever the
 * number of ports (a scheduler needs the pattern of a wider, e.g. zero-power, resource to reserve its REs).
 * SRS_AMD_EINVAL where the reference asserts (csi_rs_pattern.cpp:34-367): row 0 or > 12, a k_ref count other than the
 * row's, a k_ref outside the row's range, a density or CDM type the row does not have; also for a pattern symbol
 * at or beyond 14 (the reference's symbol mask has 14 bits). */
int srs_amd_csi_rs_pattern(const srs_amd_csi_rs_config* cfg, srs_amd_csi_rs_pattern_desc* out);

/* HOST only: the REs of srs_amd_csi_rs_pattern as RE patterns, one per CDM group with distinct REs (at most
 * SRS_AMD_MAX_RE_PATTERNS), crb_mask following rb_begin and rb_stride: ready for srs_amd_pdsch_mod_config::reserved,
 * as srs_amd_ptrs_pdsch_reserved is for PT-RS.  patterns has room for SRS_AMD_MAX_RE_PATTERNS entries; *nof_patterns
 * receives the count.  SRS_AMD_EINVAL as srs_amd_csi_rs_pattern, and for PRBs beyond SRS_AMD_MAX_RB. */
int srs_amd_csi_rs_reserved(const srs_amd_csi_rs_config* cfg, srs_amd_re_pattern* patterns, uint32_t* nof_patterns);

/* HOST only: everything the map calls check for one resource on grids of nof_grid_ports x 14 x nof_subc.  The checks
 * of srs_amd_csi_rs_pattern, and SRS_AMD_EINVAL for rows 6-12 (more than four ports cannot be precoded), a row with
 * more ports than the grid, nof_rb == 0 or (start_rb + nof_rb) x 12 > nof_subc, a density-0.5 resource that occupies
 * no PRB (the reference asserts in the mapper), scrambling_id > 1023, numerology > 4, a slot_index at or beyond the
 * numerology's slots per frame, symbol_l0 >= 14. */
int srs_amd_csi_rs_validate(const srs_amd_csi_rs_config* cfg, uint32_t nof_grid_ports, uint32_t nof_subc);

/* HOST, synchronous: one resource into a host grid, cbf16 (bf16 real in the low half, bf16 imaginary in the high half
 * of a 32-bit word) [nof_ports][14][nof_subc]; every other RE is left as it is.  cfg->grid and cfg->d_grid are
 * ignored. */
int srs_amd_csi_rs_map(srs_amd_csi_rs_generator*    gen,
                       const srs_amd_csi_rs_config* cfg,
                       uint32_t*                    grid,
                       uint32_t                     nof_ports,
                       uint32_t                     nof_subc);

/* DEVICE, asynchronous on `stream`, no host synchronisation: every CSI-RS resource of a slot.  Resource i writes
 * d_grids + grid x grid_stride (cbf16 elements; [nof_grid_ports][14][nof_subc]) or its own d_grid of the same shape.
 * ONE kernel launch per call whatever the number and kinds of resources; everything is validated before the launch.
 * The descriptors go through a ring of three pinned staging buffers and one device buffer that grow to the largest
 * call met (growing one waits for the device); calls of a size already met make no host synchronisation.
 * At the REs of a CDM group every transmit port 0 .. row ports - 1 is written (zeros where the weights are zero, as the
 * reference); grid ports beyond the row's and all other REs are untouched.  A resource's REs do not depend on its
 * position in the call, on the other resources or on the stream.
 * Two resources of one call that share an RE on one grid are the caller's error: the value at that RE is
 * UNSPECIFIED (either resource's; the reference, called twice, leaves the later call's value). */
int srs_amd_csi_rs_map_slot(srs_amd_csi_rs_generator*    gen,
                            const srs_amd_csi_rs_config* cfgs,
                            uint32_t                     nof_resources,
                            uint32_t*                    d_grids,
                            uint64_t                     grid_stride,
                            uint32_t                     nof_grids,
                            uint32_t                     nof_grid_ports,
                            uint32_t                     nof_subc,
                            void*                        stream);

#ifdef __cplusplus
}
#endif

#endif /* SRSRAN_AMD_CSI_RS_H */
