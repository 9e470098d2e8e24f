// pdsch_encoder.hip -- the PDSCH encoder chain of pdsch_encoder_impl::encode
// (lib/phy/upper/channel_processors/pdsch/pdsch_encoder_impl.cpp:28-80):
//   pdsch_cb_kernel      one wave per codeblock, everything in LDS:
//                          segmentation (ldpc_segmenter_tx_impl.cpp:137-207): the message straight from the TB;
//                          the TB CRC (CRC16 / CRC24A, crc_calculator_generic_impl.cpp), which is linear in the TB's
//                            bits: a codeblock that is not its TB's last divides its segment by the CRC24A byte
//                            table in the pass that computes its CRC24B and stores the remainder in
//                            tb_parts[TB][segment] -- every slot written on every call, no accumulator to reset, no
//                            atomics; the TB's last codeblock moves each partial to the TB end (crc_device.h), XORs
//                            them with the remainder of its own data bits and attaches the checksum after them;
//                          the CRC24B of segmented TBs (ldpc_segmenter_tx_impl.cpp:196), byte table in LDS;
//                          LDPC encoding (ldpc_encoder_impl.cpp:44-80) by the bit-sliced core (ldpc_encode_device.h)
//                            with the lifted graph staged in LDS, only the circular-buffer window the rate matcher
//                            reads;
//                          rate matching + bit interleaving (ldpc_rate_matcher_impl.cpp:95-160) into the codeword:
//                            whole bytes stored, the bytes shared with the neighbouring segments written with AND / OR
//                            atomics on the segment's own bits (the codeword's padding bits cleared by the TB's last
//                            segment), so no zeroing pass is needed.
// Two launches on the caller's stream (launch_pdsch_fused): every codeblock but the TBs' last ones (skipped when no TB
// is segmented), then the TBs' last codeblocks, one per TB.  Stream order is the only synchronisation: no workgroup
// waits for another inside a launch.  (Gathering the TB CRC inside one launch through a last-arriving workgroup needs
// an agent-scope fence per codeblock, which on the multi-XCD MI355X writes back / invalidates L2 and measured twice
// as slow.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "crc_device.h"
#include "ldpc_codec_args.h"
#include "ldpc_common.h"
#include "ldpc_encode_device.h"
#include "rate_match_device.h"
#include "sch_args.h"

namespace srs_amd {
namespace {

constexpr uint32_t PE_CW_BYTES  = 66 * MAX_LIFTING_SIZE / 8; // circular buffer of BG1, Z = 384
constexpr uint32_t PE_ENC_WORDS = enc_bits_lds_words(22, 46, MAX_LIFTING_SIZE);

// Output byte b of the segment (bits [off, off + E) of the codeword): the bits of this segment, zeros elsewhere.
__device__ __forceinline__ uint32_t pe_out_byte(const uint8_t* s_cw, const rm_geometry& g, const fast_div& divL,
                                                uint32_t off, uint32_t E, uint32_t Kq, uint32_t b)
{
  uint32_t byte = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    const uint32_t gbit = 8 * b + k;
    if (gbit < off || gbit >= off + E) {
      continue;
    }
    const uint32_t o = gbit - off;
    uint32_t       i, j;
    if (g.Qm == 6) {
      i = __umulhi(o >> 1, 0xAAAAAAABu) >> 1;
      j = o - 6 * i;
    } else {
      const uint32_t sh = g.Qm == 8 ? 3 : g.Qm == 4 ? 2 : g.Qm == 2 ? 1 : 0;
      i                 = o >> sh;
      j                 = o & (g.Qm - 1);
    }
    uint32_t w = g.rank0 + j * Kq + i;
    if (w >= g.L) {
      w -= g.L;
      if (w >= g.L) {
        divL.div(w, w); // repetition beyond one more turn
      }
    }
    const uint32_t p = w < g.nof_info ? w : w + g.F;
    byte |= ((s_cw[p >> 3] >> (7 - (p & 7))) & 1u) << (7 - k);
  }
  return byte;
}

struct pe_lds {
  uint32_t T24b[256]; // CRC24B byte table
  uint32_t Ttb[256];  // byte table of the TB CRC polynomial in use (tb_order / tb_poly)
  uint32_t lw[PE_ENC_WORDS];
  uint32_t edges[MAX_EDGES]; // the codeblock's lifted graph (the rows the encoder computes)
  // the message (MSB-first bytes), then the encoded circular-buffer window (+ the second byte of a two-byte read)
  __attribute__((aligned(16))) uint8_t s_cw[PE_CW_BYTES + 8];
  uint32_t partial[4]; // block reductions (NT > 64)
};

// XOR of v over the NT threads of the block (to every thread).
template <int NT>
__device__ __forceinline__ uint32_t pe_xor(uint32_t v, uint32_t* partial)
{
  if constexpr (NT == 64) {
    return crc_wave_xor(v);
  } else {
    return crc_block_xor<NT>(v, partial);
  }
}

// The segment of codeblock row `cb` (its TB's data bits only: zero from the data end) into s_cw as MSB-first bytes,
// K Z bits in all.
template <int NT>
__device__ __forceinline__ void pe_message(const pdsch_fused_args& a, const tb_desc& d, uint32_t r, uint32_t n_data,
                                           uint32_t kz, uint8_t* s_cw, uint32_t j)
{
  const uint8_t* tb  = a.tbs + d.tb_offset;
  const uint32_t ob  = r * d.cb_info_bits; // first TB bit of the segment
  const uint32_t nmb = (kz + 7) / 8;
  if ((ob & 7u) == 0) {
    // byte-aligned segment: message word q = TB bytes B .. B + 3 (B = ob / 8 + 4q), one funnel shift of the two
    // aligned dwords that hold them; the partial / last words below
    const uintptr_t base  = reinterpret_cast<uintptr_t>(tb) + ob / 8;
    const uint32_t  nfull = n_data / 32;
    for (uint32_t q = j; q < nfull; q += NT) {
      const uintptr_t  addr = base + 4 * q;
      const uint32_t*  p4   = reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
      const uint32_t   sh   = static_cast<uint32_t>(addr & 3u);
      const uint32_t   lo   = p4[0];
      const uint32_t   hi   = sh != 0 ? p4[1] : 0u;
      reinterpret_cast<uint32_t*>(s_cw)[q] = sh != 0 ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
    }
    for (uint32_t q = nfull + j; q < (nmb + 3) / 4; q += NT) {
      uint32_t w = 0;
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t jb = 4 * q + b;
        uint32_t       v  = 0;
        for (uint32_t k = 0; k < 8 && 8 * jb + k < n_data; ++k) {
          const uint32_t p = ob + 8 * jb + k;
          v |= ((tb[p >> 3] >> (7 - (p & 7))) & 1u) << (7 - k);
        }
        w |= v << (8 * b);
      }
      reinterpret_cast<uint32_t*>(s_cw)[q] = w;
    }
    return;
  }
  for (uint32_t q = j; q < (nmb + 3) / 4; q += NT) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
      const uint32_t jb = 4 * q + b;
      uint32_t       v  = 0;
      if (8 * jb + 8 <= n_data) {
        // 8 TB bits: one or two byte loads
        const uint32_t p  = ob + 8 * jb;
        const uint32_t sh = p & 7u;
        uint32_t       x  = static_cast<uint32_t>(tb[p >> 3]) << 8;
        if (sh != 0) {
          x |= tb[(p >> 3) + 1];
        }
        v = (x >> (8 - sh)) & 0xffu;
      } else if (8 * jb < n_data) {
        for (uint32_t k = 0; k < 8 && 8 * jb + k < n_data; ++k) {
          const uint32_t p = ob + 8 * jb + k;
          v |= ((tb[p >> 3] >> (7 - (p & 7))) & 1u) << (7 - k);
        }
      }
      w |= v << (8 * b);
    }
    reinterpret_cast<uint32_t*>(s_cw)[q] = w;
  }
}

// This thread's contributions to two 24-bit CRCs of the n-bit message in s_cw (MSB-first bytes) from its bytes
// [b0, b1): crc_chunk_contrib twice (polynomial, linear table, byte table in LDS per CRC), as two independent division
// chains over one fetch of the bytes.
__device__ __forceinline__ void pe_crc24_pair(const uint8_t* s_cw, uint32_t b0, uint32_t b1, uint32_t n,
                                              uint32_t polyA, const uint32_t* tableA, const uint32_t* TA,
                                              uint32_t polyB, const uint32_t* tableB, const uint32_t* TB,
                                              uint32_t& outA, uint32_t& outB)
{
  outA = 0;
  outB = 0;
  if (b0 >= b1) {
    return;
  }
  constexpr uint32_t highbit = 1u << 24, mask = highbit - 1u;
  const uint32_t     full    = min(b1, n / 8); // whole bytes
  uint32_t           rA = 0, rB = 0;
  for (uint32_t b = b0; b < full; b += CRC_FETCH_BATCH) {
    uint32_t v[CRC_FETCH_BATCH];
#pragma unroll
    for (uint32_t k = 0; k < CRC_FETCH_BATCH; ++k) {
      v[k] = b + k < full ? s_cw[b + k] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < CRC_FETCH_BATCH; ++k) {
      if (b + k < full) {
        rA = TA[rA >> 16] ^ ((rA << 8) & mask) ^ v[k];
        rB = TB[rB >> 16] ^ ((rB << 8) & mask) ^ v[k];
      }
    }
  }
  for (uint32_t b = max(b0, full); b < b1; ++b) {
    const uint32_t byte = s_cw[b];
    const int      nb   = (b * 8 + 8 <= n) ? 8 : static_cast<int>(n - b * 8);
    for (int i = 0; i < nb; ++i) {
      const uint32_t bit = (byte >> (7 - i)) & 1u;
      rA                 = (rA << 1) | bit;
      rB                 = (rB << 1) | bit;
      rA ^= (rA & highbit) ? polyA : 0u;
      rB ^= (rB & highbit) ? polyB : 0u;
    }
  }
  // both remainders to the message end (table[k] = x^(k + 24) mod g)
  const uint32_t  e  = min(n, b1 * 8);
  const uint32_t* ta = tableA + (n - e);
  const uint32_t* tb = tableB + (n - e);
#pragma unroll
  for (uint32_t j = 0; j < 24; ++j) {
    outA ^= ta[j] & (0u - ((rA >> j) & 1u));
    outB ^= tb[j] & (0u - ((rB >> j) & 1u));
  }
}

// CRC24B (C > 1), LDPC encoding and rate matching of codeblock row `cb` (segment r of TB t) whose message is in s_cw.
// A segment that is not its TB's last also stores its contribution to the TB CRC in tb_parts[t][r].
// staged_off / staged_ne: the lifted graph s.edges holds (a workgroup that goes on to a codeblock of the same graph and
// window, as every codeblock of a uniform batch is, keeps it).
template <int NT>
__device__ __forceinline__ void pe_finish(const pdsch_fused_args& a, pe_lds& s, uint32_t cb, uint32_t t,
                                          const tb_desc& d, uint32_t j, uint32_t& staged_off, uint32_t& staged_ne)
{
  const rm_geometry  g   = a.geos[a.row_geo[cb]];
  const enc_row_desc er  = a.enc_rows[cb];
  const uint32_t     E   = a.row_E[cb];
  const uint32_t     off = a.row_out[cb];
  const uint32_t     Z   = er.Z;
  const uint32_t     Kb  = g.nof_sys / Z + 2;
  const int          bg  = Kb == 22 ? 1 : 2;
  const uint32_t     kz  = Kb * Z;
  uint8_t*           s_cw = s.s_cw;
  // ---- CRC24B of segmented TBs over the cbi message bits, attached MSB-first after them
  if (d.nof_segments > 1) {
    const uint32_t cbi = d.cb_info_bits;
    const uint32_t nb  = (cbi + 7) / 8;
    const uint32_t per = (nb + NT - 1) / NT;
    const uint32_t b0  = j * per;
    const uint32_t r   = cb - d.row0;
    uint32_t       crc;
    if (r + 1 < d.nof_segments) {
      // the same bits are TB bits [r cbi, (r + 1) cbi): their CRC24A remainder (times x^24); the TB's last codeblock
      // moves it to the TB end
      uint32_t tb_part;
      pe_crc24_pair(s_cw, b0, min(nb, b0 + per), cbi, a.crc24b_poly, a.crc24b_table, s.T24b, a.crc24a_poly,
                    a.crc24a_table, s.Ttb, crc, tb_part);
      crc     = pe_xor<NT>(crc, s.partial);
      tb_part = pe_xor<NT>(tb_part, s.partial);
      if (j == 0) {
        a.tb_parts[static_cast<size_t>(t) * a.part_stride + r] = tb_part;
      }
    } else {
      crc = pe_xor<NT>(crc_chunk_contrib(lds_chunk_fetch{s_cw, 0}, b0, min(nb, b0 + per), cbi, 24, a.crc24b_poly,
                                         a.crc24b_table, s.T24b),
                       s.partial);
    }
    if (j == 0) {
      attach_crc_bits(s_cw, cbi, 24, crc);
    }
    __syncthreads();
  }
  // ---- message words of the bit-linear codeword (bit i at word i / 32, bit i % 32), the rest zeroed
  const uint32_t nq  = (Z + 31) / 32;
  const uint32_t ncw = enc_bits_cw_words(Kb, er.M_eff, Z);
  uint32_t*      cwb = s.lw;
  uint32_t*      lam = s.lw + ncw;
  uint32_t*      ls  = lam + 4 * nq;
  const uint32_t nmw = (kz + 31) / 32;
  for (uint32_t w = j; w < ncw; w += NT) {
    uint32_t v = 0;
    if (w < nmw) {
      v = __builtin_bitreverse32(__builtin_bswap32(reinterpret_cast<const uint32_t*>(s_cw)[w]));
      if (32 * w + 32 > kz) {
        v &= (1u << (kz - 32 * w)) - 1u;
      }
    }
    cwb[w] = v;
  }
  for (uint32_t w = j; w < nq + 2; w += NT) {
    ls[w] = 0;
  }
  const uint32_t* ge = a.edges + er.edge_off;
  const uint32_t  ne = static_cast<uint32_t>(a.row_start[bg - 1][er.M_eff]);
  if (er.edge_off != staged_off || ne != staged_ne) {
    for (uint32_t e = j; e < ne; e += NT) {
      s.edges[e] = ge[e];
    }
    staged_off = er.edge_off;
    staged_ne  = ne;
  }
  __syncthreads();
  // ---- parity of the encoded window (edge descriptors from LDS: every edge read is then an LDS latency)
  const int32_t core_a[3] = {static_cast<int32_t>(er.core_a[0]), static_cast<int32_t>(er.core_a[1]),
                             static_cast<int32_t>(er.core_a[2])};
  encode_bits_parity<NT>(cwb, lam, ls, s.edges, a.row_start[bg - 1], bg, Kb, Z, er.M_eff,
                                 static_cast<int32_t>(er.p0_shift), core_a, j);
  // ---- the shortened codeword window (from bit 2Z) as MSB-first bytes into s_cw
  const uint32_t nbits = er.pack_bits;
  for (uint32_t m = j; m < (nbits + 31) / 32; m += NT) {
    uint32_t v = lds_bits32(cwb, 2 * Z + 32 * m);
    if (32 * m + 32 > nbits) {
      v &= (1u << (nbits - 32 * m)) - 1u;
    }
    reinterpret_cast<uint32_t*>(s_cw)[m] = __builtin_bswap32(__builtin_bitreverse32(v));
  }
  __syncthreads();
  // ---- rate matching + bit interleaving into codeword bits [off, off + E)
  const fast_div divL(g.L);
  const uint32_t Kq    = E / g.Qm;
  const uint32_t first = (off + 7) / 8;
  const uint32_t whole = (off + E) / 8; // bytes [first, whole) hold only bits of this segment
  // groups of 8 symbols (Qm bytes each) of a byte-aligned segment
  const uint32_t G        = ((off & 7u) == 0 && g.Qm >= 2) ? Kq / 8 : 0;
  const uint32_t fast_end = first + G * g.Qm;
  for (uint32_t gi = j; gi < G; gi += NT) {
    uint64_t x = 0;
#pragma unroll
    for (uint32_t jj = 0; jj < 8; ++jj) {
      if (jj < g.Qm) {
        uint32_t w = g.rank0 + jj * Kq + 8 * gi;
        if (w >= g.L) {
          w -= g.L;
          if (w >= g.L) {
            divL.div(w, w);
          }
        }
        x |= static_cast<uint64_t>(rm_walk_byte(s_cw, g, w)) << (56 - 8 * jj);
      }
    }
    x            = transpose8x8(x);
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
      acc = (acc << g.Qm) | ((x >> (64 - 8 * q - g.Qm)) & ((1u << g.Qm) - 1u));
    }
    uint8_t* o = a.cw + first + gi * g.Qm;
    for (uint32_t q = 0; q < g.Qm; ++q) {
      o[q] = static_cast<uint8_t>(acc >> (8 * (g.Qm - 1 - q)));
    }
  }
  for (uint32_t b = fast_end + j; b < whole; b += NT) {
    a.cw[b] = static_cast<uint8_t>(pe_out_byte(s_cw, g, divL, off, E, Kq, b));
  }
  // bytes shared with the previous / next segment: clear this segment's bits (and, for the TB's last segment, the
  // codeword's padding bits after them), then set its ones -- the neighbour's bits are never touched
  if (j < 2) {
    const bool     last_seg = cb == d.row0 + d.nof_segments - 1;
    const uint32_t b        = j == 0 ? off / 8 : whole;
    // (j = 1: the end byte, unless it is the start byte that j = 0 already covers)
    const bool partial =
        j == 0 ? (off & 7u) != 0 : ((off + E) & 7u) != 0 && (whole != off / 8 || (off & 7u) == 0);
    if (partial) {
      uint32_t mask = 0;
      for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t gbit = 8 * b + k;
        mask |= (gbit >= off && (gbit < off + E || last_seg)) ? (0x80u >> k) : 0u;
      }
      const uint32_t v  = pe_out_byte(s_cw, g, divL, off, E, Kq, b);
      uint32_t*      w4 = reinterpret_cast<uint32_t*>(a.cw + (b & ~3u));
      const uint32_t sh = 8 * (b & 3u);
      atomicAnd(w4, ~(mask << sh));
      atomicOr(w4, v << sh);
    }
  }
  __syncthreads(); // s_cw / lw are rewritten by the next codeblock
}

template <int NT>
__global__ __launch_bounds__(NT) void pdsch_cb_kernel(pdsch_fused_args a)
{
  __shared__ pe_lds s;
  // byte tables, once per workgroup: CRC24B, and the TB CRC's (CRC24A; a CRC16 TB rebuilds it below)
  crc_table8_init<NT>(s.T24b, 24, a.crc24b_poly);
  crc_table8_init<NT>(s.Ttb, 24, a.crc24a_poly);
  uint32_t       tb_table_order = 24;
  uint32_t       staged_off = 0, staged_ne = 0; // s.edges: nothing staged
  const uint32_t j              = threadIdx.x;

  // last_only 0: every codeblock but the TBs' last ones (each stores its TB CRC partial); 1: the TBs' last codeblocks
  // (a.last_rows, one per TB), launched after the others in stream order, so the partials are in
  const uint32_t n = a.last_only == 1 ? a.nof_tbs : a.nof_cbs;
  for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
    const uint32_t cb   = a.last_only == 1 ? a.last_rows[k] : k;
    const uint32_t t    = a.row_tb[cb];
    const tb_desc  d    = a.tds[t];
    const uint32_t r    = cb - d.row0;
    const uint32_t C    = d.nof_segments;
    const bool     last = r == C - 1;
    if ((a.last_only == 0) == last) {
      continue; // uniform over the workgroup
    }
    const uint32_t L    = d.tb_crc_bits;
    // TB data bits of the segment (the last one: up to the TB CRC; a plan may count that CRC outside cb_info_bits,
    // as pdsch_encoder_hw_impl's single segment does)
    const uint32_t n_data = last ? d.cb_info_bits - L - d.zero_pad : d.cb_info_bits;
    const uint32_t kz     = (a.geos[a.row_geo[cb]].nof_sys / a.enc_rows[cb].Z + 2) * a.enc_rows[cb].Z;
    // ---- 1. the segment's TB data bits; the last segment: the TB CRC after them, the XOR of the other segments'
    // partials and of the contribution of its own data bits (they end where the TB ends)
    uint32_t tb_crc = 0;
    if (last) {
      if (tb_table_order != L) {
        // (s.Ttb is not read between the barrier that ends the previous codeblock and the one after pe_message)
        crc_table8_init<NT>(s.Ttb, L, L == 16 ? a.crc16_poly : a.crc24a_poly);
        tb_table_order = L;
      }
      for (uint32_t i = j; i + 1 < C; i += NT) {
        // segment i's remainder, times x^(TB bits after the segment) (C > 1: CRC24A)
        tb_crc ^= crc_move(a.tb_parts[static_cast<size_t>(t) * a.part_stride + i],
                           d.tbs_bits - (i + 1) * d.cb_info_bits, 24, a.crc24a_table);
      }
    }
    pe_message<NT>(a, d, r, n_data, kz, s.s_cw, j);
    __syncthreads();
    if (last) {
      const uint32_t nb  = (n_data + 7) / 8;
      const uint32_t per = (nb + NT - 1) / NT;
      const uint32_t b0  = j * per;
      tb_crc ^= crc_chunk_contrib(lds_chunk_fetch{s.s_cw, 0}, b0, min(nb, b0 + per), n_data, L,
                                  L == 16 ? a.crc16_poly : a.crc24a_poly, L == 16 ? a.crc16_table : a.crc24a_table,
                                  s.Ttb);
      tb_crc = pe_xor<NT>(tb_crc, s.partial);
      if (j == 0) {
        attach_crc_bits(s.s_cw, n_data, L, tb_crc); // zero padding stays zero after it
      }
      __syncthreads();
    }
    // ---- 2. CB CRC (with the TB CRC partial of a segment that is not the last), encoding, rate matching
    pe_finish<NT>(a, s, cb, t, d, j, staged_off, staged_ne);
  }
}

constexpr int PE_MAX_DEVICES = 64;

// Workgroups of pdsch_cb_kernel<NT> that are resident on the current device at once (by its registers and LDS).
template <int NT>
uint32_t pe_resident_workgroups()
{
  static std::atomic<uint32_t> known[PE_MAX_DEVICES] = {}; // per device, asked once
  int                          dev = 0, per_cu = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PE_MAX_DEVICES) {
    (void)hipGetLastError();
    return 65535u;
  }
  uint32_t n = known[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0 ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pdsch_cb_kernel<NT>, NT, 0) != hipSuccess ||
        per_cu <= 0) {
      (void)hipGetLastError();
      return 65535u;
    }
    n = static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(cus);
    known[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

} // namespace

hipError_t launch_pdsch_fused(const pdsch_fused_args& a, hipStream_t stream)
{
  if (a.nof_cbs == 0) {
    return hipSuccess;
  }
  // threads per codeblock: SRSRAN_AMD_PDSCH_WG (read per launch) 256, else one wave.  The TBs' last codeblocks are
  // one workgroup per TB, so that launch lasts as long as its slowest codeblock: four waves each (a low-rate Z = 384
  // codeblock takes 36 us so, 72 us with one wave), SRSRAN_AMD_PDSCH_TAIL_WG=64: one wave
  const char* wg       = std::getenv("SRSRAN_AMD_PDSCH_WG");
  const char* tail     = std::getenv("SRSRAN_AMD_PDSCH_TAIL_WG");
  const bool  big      = wg != nullptr && wg[0] == '2';
  const bool  big_tail = tail == nullptr || tail[0] == '2';
  // workgroups of the first launch: as many as stay resident, each looping over its codeblocks with the byte tables
  // built and the lifted graph staged once (SRSRAN_AMD_PDSCH_GRID: that many instead; 65535: one per codeblock)
  const char*    gs  = std::getenv("SRSRAN_AMD_PDSCH_GRID");
  const uint32_t cap = gs != nullptr && std::atoi(gs) > 0 ? static_cast<uint32_t>(std::atoi(gs))
                       : big                              ? pe_resident_workgroups<256>()
                                                          : pe_resident_workgroups<64>();
  auto cb_launch = [&](uint32_t last_only, uint32_t n, bool wide) {
    pdsch_fused_args x = a;
    x.last_only        = last_only;
    const dim3 grid(std::min(n, last_only == 0 ? std::min(cap, 65535u) : 65535u));
    if (wide) {
      hipLaunchKernelGGL(pdsch_cb_kernel<256>, grid, dim3(256), 0, stream, x);
    } else {
      hipLaunchKernelGGL(pdsch_cb_kernel<64>, grid, dim3(64), 0, stream, x);
    }
  };
  if (a.nof_cbs > a.nof_tbs) {
    // every codeblock but the TBs' last ones: each stores its TB CRC partial
    cb_launch(0, a.nof_cbs, big);
  }
  // the TBs' last codeblocks, after the partials in stream order
  cb_launch(1, a.nof_tbs, big_tail);
  return hipGetLastError();
}

} // namespace srs_amd
