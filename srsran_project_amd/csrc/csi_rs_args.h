// csi_rs_args.h -- per-wave descriptor of the NZP-CSI-RS kernel (csi_rs.hip), shared with the C-ABI (csi_rs_api.cpp),
// which validates every field before the launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "srsran_amd/csi_rs.h"

namespace srs_amd {

constexpr uint32_t CSI_RS_NSYMB       = 14;
constexpr uint32_t CSI_RS_MAX_PORTS   = SRS_AMD_CSI_RS_MAX_PORTS;
constexpr uint32_t CSI_RS_GROUP_PORTS = 2;   // fd-CDM2: the widest CDM group of rows 1-5
constexpr uint32_t CSI_RS_MAX_SEQ_LEN = 825; // row 1 on 275 PRB: 52 Gold words, one per lane of a wave

// One (resource, CDM group): the group's single OFDM symbol (rows 1-5 have no time-domain CDM).
struct csi_rs_item {
  uint32_t* grid;       // cbf16 [nof_grid_ports][14][nof_subc]
  uint32_t  c_init;     // TS 38.211 7.4.1.5.2, already mod 2^31
  uint32_t  skip_bits;  // 2 x get_nof_skipped_elements
  uint32_t  seq_len;    // elements of the symbol: occupied PRBs x per_prb
  uint32_t  first_subc; // 12 x the first occupied PRB
  uint32_t  prb_step;   // 12 (density one or three) or 24 (density 0.5)
  uint32_t  per_prb;    // elements per PRB: 3 (row 1), 1 (row 2), 2 (fd-CDM2)
  uint32_t  k_bar;      // first subcarrier of the group within the PRB
  uint32_t  k_step;     // 4 (row 1) or 1
  uint32_t  symbol;
  uint32_t  nof_subc;
  uint32_t  group_size; // 1 or 2 ports
  uint32_t  nof_tx;     // the row's ports: transmit ports 0 .. nof_tx - 1 are written
  uint32_t  bypass;     // one port with weight exactly 1.0: no product
  float     amplitude;  // float(M_SQRT1_2 x amplitude), the product in double
  float     w[CSI_RS_GROUP_PORTS][CSI_RS_MAX_PORTS][2]; // [port of the group][tx port] (re, im)
};

// One wave per item, four waves per workgroup; jump: gold_jump_tables().
hipError_t launch_csi_rs_map(const csi_rs_item* items, uint32_t nof_items, const uint32_t* jump, hipStream_t stream);

} // namespace srs_amd
