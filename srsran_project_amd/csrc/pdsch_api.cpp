// pdsch_api.cpp -- C-ABI of the MI355X PDSCH encoder (include/srsran_amd/sch.h),
// pdsch_encoder_impl::encode (lib/phy/upper/channel_processors/pdsch/pdsch_encoder_impl.cpp:28-80)
// for a batch of transport blocks (srs_amd_pdsch_encode_batch) or a slot of heterogeneous ones
// (srs_amd_pdsch_encode_slot), both as the two launches of pdsch_encoder.hip:
//   1. segmentation, CB CRC24B, LDPC encoding,    pdsch_cb_kernel   over every codeblock but the TBs' last; each
//      rate matching + concatenation                                also stores its partial of the TB CRC
//   2. the TBs' last codeblocks (TB CRC = XOR of  pdsch_cb_kernel   after 1. in stream order
//      the partials and of their own bits)
// The two forms differ only in how the host builds the descriptors (encoder_rows) the kernel reads.  The encoder owns
// CRC calculators and an LDPC encoder for their device tables (CRC tables, lifted edges), not to call them.
#include "srsran_amd/crc.h"
#include "srsran_amd/ldpc_encoder.h"
#include "srsran_amd/sch.h"

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "crc_internal.h"
#include "device_buffer.h"
#include "ldpc_codec_args.h"
#include "ldpc_common.h"
#include "ldpc_codec_internal.h"
#include "rate_matching_common.h"
#include "sch_args.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

using namespace srs_amd;

struct srs_amd_pdsch_encoder {
  int                        device = 0;
  hipStream_t                stream = nullptr;
  srs_amd_crc_calculator*    crc16  = nullptr;
  srs_amd_crc_calculator*    crc24a = nullptr;
  srs_amd_crc_calculator*    crc24b = nullptr;
  srs_amd_ldpc_encoder*      enc    = nullptr;
  device_buffer              host_io, slot_desc;
  device_buffer              batch_desc, tb_parts; // uniform-batch descriptors, TB CRC partials
  std::vector<uint8_t>       batch_key;            // the batch whose descriptors batch_desc holds
  stream_order               order;  // scratch reuse across the callers' streams
  std::mutex                 mtx;
  pinned_stage               hstage; // descriptors staged in pinned memory (a ring: each reused once uploaded)
  ~srs_amd_pdsch_encoder()
  {
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    srs_amd_crc_calculator_destroy(crc16);
    srs_amd_crc_calculator_destroy(crc24a);
    srs_amd_crc_calculator_destroy(crc24b);
    srs_amd_ldpc_encoder_destroy(enc);
  }
};

namespace {

int check_plan(const srs_amd_sch_plan* p)
{
  if (p == nullptr || p->nof_segments == 0 || p->lifting_size == 0) {
    return fail(SRS_AMD_EINVAL, "plan not computed (srs_amd_sch_plan_compute)");
  }
  return SRS_AMD_OK;
}

// Host descriptors of one launch pair (pdsch_fused_args).
struct encoder_rows {
  std::vector<tb_desc>      tds;
  std::vector<uint32_t>     row_E, row_out, row_geo, row_tb;
  std::vector<rm_geometry>  geos;
  std::vector<enc_row_desc> enc;
  uint32_t                  max_segments = 0;
};

struct desc_layout {
  size_t o_E, o_out, o_geo, o_tb, o_G, o_TD, o_ER, o_LR, total;
  explicit desc_layout(const encoder_rows& f)
  {
    const size_t R = f.row_E.size();
    o_E            = 0;
    o_out          = o_E + align_up(sizeof(uint32_t) * R, 16);
    o_geo          = o_out + align_up(sizeof(uint32_t) * R, 16);
    o_tb           = o_geo + align_up(sizeof(uint32_t) * R, 16);
    o_G            = o_tb + align_up(sizeof(uint32_t) * R, 16);
    o_TD           = o_G + align_up(sizeof(rm_geometry) * f.geos.size(), 16);
    o_ER           = o_TD + align_up(sizeof(tb_desc) * f.tds.size(), 16);
    o_LR           = o_ER + align_up(sizeof(enc_row_desc) * R, 16);
    total          = o_LR + sizeof(uint32_t) * f.tds.size();
  }
};

// Appends the codeblock rows of one transport block (plan p, TB bytes at tb_offset, codeword at bit cw_bit) with
// rate-matching geometry index geo.
void add_tb(encoder_rows& f, const srs_amd_sch_plan* p, uint64_t tb_offset, uint64_t cw_bit, uint32_t geo,
            const enc_row_desc& er, std::vector<uint32_t>& segE, std::vector<uint32_t>& segOff)
{
  const uint32_t row0 = static_cast<uint32_t>(f.row_E.size());
  const uint32_t t    = static_cast<uint32_t>(f.tds.size());
  f.tds.push_back(tb_desc{tb_offset, row0, p->nof_segments, p->cb_info_bits, p->tbs, p->nof_tb_crc_bits, p->zero_pad,
                          (p->segment_length + 7) / 8, 0});
  segE.resize(p->nof_segments);
  segOff.resize(p->nof_segments);
  (void)srs_amd_sch_plan_segments(p, segE.data(), segOff.data());
  for (uint32_t r = 0; r < p->nof_segments; ++r) {
    f.row_E.push_back(segE[r]);
    f.row_out.push_back(static_cast<uint32_t>(cw_bit) + segOff[r]);
    f.row_geo.push_back(geo);
    f.row_tb.push_back(t);
    f.enc.push_back(er);
  }
  f.max_segments = std::max(f.max_segments, p->nof_segments);
}

// Encoder row descriptor of plan p: lifted graph and the circular-buffer window [0, k0 + E + F) the rate matcher
// reads (ldpc_rate_matcher_impl.cpp:95-130), capped at Ncb.
enc_row_desc enc_row_of(const srs_amd_sch_plan* p, const rm_geometry& g)
{
  const uint64_t window = static_cast<uint64_t>(g.k0) + std::max(p->rm_length_long, p->rm_length_short) + g.F;
  enc_row_desc   er{};
  ldpc_encode_row_desc(&er, p->base_graph, p->lifting_size, window >= g.Ncb ? g.Ncb : static_cast<uint32_t>(window));
  return er;
}

// Writes the descriptors to dd (device) from the pinned staging buffer when `upload`, then runs the two launches on
// stream (launch_pdsch_fused).
int launch_locked(srs_amd_pdsch_encoder* e,
                  const encoder_rows&    f,
                  uint8_t*               dd,
                  bool                   upload,
                  const uint8_t*         d_tbs,
                  uint8_t*               d_cw,
                  hipStream_t            stream)
{
  static const auto row_starts = [] {
    std::vector<int32_t> rs(2 * 47, 0);
    for (int bg = 1; bg <= 2; ++bg) {
      lifted_graph g{};
      build_lifted_graph(g, bg, 2);
      std::copy(g.row_start, g.row_start + g.M + 1, rs.begin() + 47 * (bg - 1));
    }
    return rs;
  }();
  const desc_layout L(f);
  const uint32_t    U           = static_cast<uint32_t>(f.tds.size());
  const uint32_t    R           = static_cast<uint32_t>(f.row_E.size());
  const uint32_t    part_stride = std::max(2u, f.max_segments) - 1; // a partial per codeblock but the TB's last
  hipError_t        he          = e->tb_parts.ensure(sizeof(uint32_t) * U * part_stride);
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH encoder TB CRC partials");
  }
  call_scope scope(e->order, nullptr, stream);
  he = e->order.begin(stream);
  if (he == hipSuccess && upload) {
    // the next pinned staging buffer of the ring, free once its previous upload completed
    he = e->hstage.acquire(L.total);
    if (he == hipSuccess) {
      auto* h = e->hstage.at<uint8_t>(0);
      std::memcpy(h + L.o_E, f.row_E.data(), sizeof(uint32_t) * R);
      std::memcpy(h + L.o_out, f.row_out.data(), sizeof(uint32_t) * R);
      std::memcpy(h + L.o_geo, f.row_geo.data(), sizeof(uint32_t) * R);
      std::memcpy(h + L.o_tb, f.row_tb.data(), sizeof(uint32_t) * R);
      std::memcpy(h + L.o_G, f.geos.data(), sizeof(rm_geometry) * f.geos.size());
      std::memcpy(h + L.o_TD, f.tds.data(), sizeof(tb_desc) * U);
      std::memcpy(h + L.o_ER, f.enc.data(), sizeof(enc_row_desc) * R);
      auto* lr = reinterpret_cast<uint32_t*>(h + L.o_LR);
      for (uint32_t t = 0; t < U; ++t) {
        lr[t] = f.tds[t].row0 + f.tds[t].nof_segments - 1;
      }
      he = e->hstage.upload(dd, L.total, stream);
    }
  }
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH encoder descriptors upload");
  }
  pdsch_fused_args a{};
  a.tbs          = d_tbs;
  a.tds          = reinterpret_cast<const tb_desc*>(dd + L.o_TD);
  a.row_tb       = reinterpret_cast<const uint32_t*>(dd + L.o_tb);
  a.row_E        = reinterpret_cast<const uint32_t*>(dd + L.o_E);
  a.row_out      = reinterpret_cast<const uint32_t*>(dd + L.o_out);
  a.row_geo      = reinterpret_cast<const uint32_t*>(dd + L.o_geo);
  a.geos         = reinterpret_cast<const rm_geometry*>(dd + L.o_G);
  a.enc_rows     = reinterpret_cast<const enc_row_desc*>(dd + L.o_ER);
  a.last_rows    = reinterpret_cast<const uint32_t*>(dd + L.o_LR);
  a.edges        = ldpc_encoder_edges(e->enc);
  a.tb_parts     = e->tb_parts.as<uint32_t>();
  a.part_stride  = part_stride;
  a.crc16_table  = crc_device_table(e->crc16);
  a.crc24a_table = crc_device_table(e->crc24a);
  a.crc24b_table = crc_device_table(e->crc24b);
  a.crc16_poly   = crc_polynom(e->crc16);
  a.crc24a_poly  = crc_polynom(e->crc24a);
  a.crc24b_poly  = crc_polynom(e->crc24b);
  a.cw           = d_cw;
  a.nof_tbs      = U;
  a.nof_cbs      = R;
  std::copy(row_starts.begin(), row_starts.begin() + 47, a.row_start[0]);
  std::copy(row_starts.begin() + 47, row_starts.end(), a.row_start[1]);
  he = launch_pdsch_fused(a, stream);
  if (he == hipSuccess) {
    he = scope.close();
  }
  return he == hipSuccess ? SRS_AMD_OK : hip_fail(he, "PDSCH encoder launch");
}

// srs_amd_pdsch_encode_batch: the descriptors of a uniform batch, uploaded again only when the batch (plan, count,
// strides) changes.
int encode_batch_locked(srs_amd_pdsch_encoder* e,
                        const srs_amd_sch_plan* p,
                        uint8_t*                d_cw,
                        uint32_t                cw_stride,
                        const uint8_t*          d_tbs,
                        uint32_t                tb_stride,
                        uint32_t                nof_tbs,
                        hipStream_t             stream)
{
  std::vector<uint8_t> key(sizeof(*p) + 3 * sizeof(uint32_t));
  std::memcpy(key.data(), p, sizeof(*p));
  const uint32_t k3[3] = {cw_stride, tb_stride, nof_tbs};
  std::memcpy(key.data() + sizeof(*p), k3, sizeof(k3));
  rm_geometry g{};
  if (const char* msg = make_rm_geometry(g, p->base_graph, p->lifting_size, p->rv, p->modulation_order, p->Nref,
                                         p->nof_filler_bits)) {
    return fail(SRS_AMD_EINVAL, "%s", msg);
  }
  encoder_rows f;
  f.geos.push_back(g);
  const enc_row_desc    er = enc_row_of(p, g);
  std::vector<uint32_t> segE, segOff;
  for (uint32_t t = 0; t < nof_tbs; ++t) {
    add_tb(f, p, static_cast<uint64_t>(t) * tb_stride, static_cast<uint64_t>(t) * cw_stride * 8, 0, er, segE,
           segOff);
  }
  const bool upload = key != e->batch_key;
  hipError_t he     = hipSetDevice(e->device);
  if (he == hipSuccess && upload) {
    he = e->batch_desc.ensure(desc_layout(f).total);
  }
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH encoder descriptors");
  }
  e->batch_key.clear();
  int rc = launch_locked(e, f, e->batch_desc.as<uint8_t>(), upload, d_tbs, d_cw, stream);
  if (rc == SRS_AMD_OK) {
    e->batch_key = std::move(key);
  }
  return rc;
}

// srs_amd_pdsch_encode_slot (every UE's plan, one launch pair).
int encode_slot_locked(srs_amd_pdsch_encoder*  e,
                       const srs_amd_pdsch_ue* ues,
                       uint32_t                U,
                       const uint8_t*          d_tbs,
                       uint8_t*                d_cw,
                       hipStream_t             stream)
{
  encoder_rows f;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t> geo_of;
  std::vector<uint32_t> segE, segOff;
  uint32_t              R = 0;
  for (uint32_t u = 0; u < U; ++u) {
    const srs_amd_sch_plan* p  = &ues[u].plan;
    int                     rc = check_plan(p);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    rm_geometry g{};
    if (const char* msg = make_rm_geometry(g, p->base_graph, p->lifting_size, p->rv, p->modulation_order, p->Nref,
                                           p->nof_filler_bits)) {
      return fail(SRS_AMD_EINVAL, "UE %u: %s", u, msg);
    }
    if ((ues[u].cw_offset + (p->cw_length + 7) / 8) * 8 > 0xffffffffull) {
      return fail(SRS_AMD_EINVAL, "UE %u: codeword span exceeds 2^32 bits", u);
    }
    R += p->nof_segments;
    if (U > 65535 || R > 65535) {
      return fail(SRS_AMD_EINVAL, "%u UEs / %u+ codeblocks exceed the 65535 of one slot batch", U, R);
    }
    const auto gkey = std::make_tuple(p->base_graph, p->lifting_size, p->rv, p->modulation_order, p->Nref,
                                      p->nof_filler_bits, 0u);
    auto       git  = geo_of.find(gkey);
    if (git == geo_of.end()) {
      git = geo_of.emplace(gkey, static_cast<uint32_t>(f.geos.size())).first;
      f.geos.push_back(g);
    }
    add_tb(f, p, ues[u].tb_offset, ues[u].cw_offset * 8, git->second, enc_row_of(p, g), segE, segOff);
  }
  hipError_t he = hipSetDevice(e->device);
  if (he == hipSuccess) {
    he = e->slot_desc.ensure(desc_layout(f).total);
  }
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH slot encoder descriptors");
  }
  return launch_locked(e, f, e->slot_desc.as<uint8_t>(), true, d_tbs, d_cw, stream);
}

} // namespace

extern "C" {

int srs_amd_pdsch_encode_slot(srs_amd_pdsch_encoder*  enc,
                              const srs_amd_pdsch_ue* ues,
                              uint32_t                nof_ues,
                              const uint8_t*          d_tbs,
                              uint8_t*                d_codewords,
                              void*                   stream)
{
  if (enc == nullptr) {
    return fail(SRS_AMD_EINVAL, "null encoder");
  }
  if (nof_ues == 0) {
    return SRS_AMD_OK;
  }
  if (ues == nullptr || d_tbs == nullptr || d_codewords == nullptr) {
    return fail(SRS_AMD_EINVAL, "null buffer");
  }
  std::lock_guard<std::mutex> lock(enc->mtx);
  return encode_slot_locked(enc, ues, nof_ues, d_tbs, d_codewords, static_cast<hipStream_t>(stream));
}

int srs_amd_pdsch_encoder_create(srs_amd_pdsch_encoder** out, int device)
{
  if (out == nullptr) {
    return fail(SRS_AMD_EINVAL, "null handle pointer");
  }
  *out   = nullptr;
  int rc = select_device(device);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  auto* e   = new srs_amd_pdsch_encoder();
  e->device = device;
  rc        = srs_amd_crc_calculator_create(&e->crc16, 3, 3824, device);
  if (rc == SRS_AMD_OK) {
    rc = srs_amd_crc_calculator_create(&e->crc24a, 0, 1277992, device);
  }
  if (rc == SRS_AMD_OK) {
    rc = srs_amd_crc_calculator_create(&e->crc24b, 1, 8448, device);
  }
  if (rc == SRS_AMD_OK) {
    rc = srs_amd_ldpc_encoder_create(&e->enc, device);
  }
  if (rc == SRS_AMD_OK) {
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) {
      rc = hip_fail(he, "PDSCH encoder stream");
    }
  }
  if (rc != SRS_AMD_OK) {
    delete e;
    return rc;
  }
  *out = e;
  return SRS_AMD_OK;
}

void srs_amd_pdsch_encoder_destroy(srs_amd_pdsch_encoder* enc)
{
  delete enc;
}

int srs_amd_pdsch_encode_batch(srs_amd_pdsch_encoder*  enc,
                               const srs_amd_sch_plan* plan,
                               uint8_t*                d_codewords,
                               uint32_t                cw_stride,
                               const uint8_t*          d_tbs,
                               uint32_t                tb_stride,
                               uint32_t                nof_tbs,
                               void*                   stream)
{
  if (enc == nullptr) {
    return fail(SRS_AMD_EINVAL, "null PDSCH encoder");
  }
  int rc = check_plan(plan);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  if (nof_tbs == 0) {
    return SRS_AMD_OK;
  }
  if (d_codewords == nullptr || d_tbs == nullptr) {
    return fail(SRS_AMD_EINVAL, "null device buffer");
  }
  if (static_cast<uint64_t>(cw_stride) * 8 < plan->cw_length || static_cast<uint64_t>(tb_stride) * 8 < plan->tbs) {
    return fail(SRS_AMD_EINVAL, "row strides too small (codeword %u bits, TB %u bits)", plan->cw_length, plan->tbs);
  }
  if (static_cast<uint64_t>(nof_tbs) * cw_stride * 8 >= (1ull << 32)) {
    return fail(SRS_AMD_EINVAL, "batch of %u codewords exceeds 2^32 bits", nof_tbs);
  }
  std::lock_guard<std::mutex> lock(enc->mtx);
  return encode_batch_locked(enc, plan, d_codewords, cw_stride, d_tbs, tb_stride, nof_tbs,
                             static_cast<hipStream_t>(stream));
}

int srs_amd_pdsch_encode(srs_amd_pdsch_encoder* enc, uint8_t* codeword, const uint8_t* transport_block,
                         const srs_amd_sch_plan* plan)
{
  if (enc == nullptr || codeword == nullptr || transport_block == nullptr) {
    return fail(SRS_AMD_EINVAL, "null argument");
  }
  int rc = check_plan(plan);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  const uint32_t tb_bytes = plan->tbs / 8;
  const uint32_t cw_bytes = (plan->cw_length + 7) / 8;
  const size_t   tb_off   = align_up(cw_bytes, 256);
  std::lock_guard<std::mutex> lock(enc->mtx);
  hipError_t                  he = hipSetDevice(enc->device);
  if (he == hipSuccess) {
    he = enc->host_io.ensure(tb_off + tb_bytes);
  }
  uint8_t* d_cw = enc->host_io.as<uint8_t>();
  uint8_t* d_tb = d_cw + tb_off;
  if (he == hipSuccess) {
    he = hipMemcpyAsync(d_tb, transport_block, tb_bytes, hipMemcpyHostToDevice, enc->stream);
  }
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH encoder upload");
  }
  rc = encode_batch_locked(enc, plan, d_cw, cw_bytes, d_tb, tb_bytes, 1, enc->stream);
  if (rc != SRS_AMD_OK) {
    return rc;
  }
  std::vector<uint8_t> packed(cw_bytes);
  he = hipMemcpyAsync(packed.data(), d_cw, cw_bytes, hipMemcpyDeviceToHost, enc->stream);
  if (he == hipSuccess) {
    he = hipStreamSynchronize(enc->stream);
  }
  if (he != hipSuccess) {
    return hip_fail(he, "PDSCH encoder download");
  }
  for (uint32_t i = 0; i < plan->cw_length; ++i) {
    codeword[i] = (packed[i >> 3] >> (7 - (i & 7))) & 1u;
  }
  return SRS_AMD_OK;
}

} // extern "C"
