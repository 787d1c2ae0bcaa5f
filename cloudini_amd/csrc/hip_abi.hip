// hip_abi.hip -- host side of the C ABI declared in include/cloudini_hip.h.
//
// Plan building restates the reference's encoder selection (src/codec_common.cpp:69-153,
// src/v4_codec.cpp:26-40, src/v5_codec.cpp:719-740, :883-892); everything else is device plumbing: a
// grow-only workspace, the chunk table of a batch, kernel launches on one HIP stream.
//
// There is no CPU implementation behind this ABI: without a GPU every call fails with
// CLDN_HIP_ERR_NO_DEVICE / CLDN_HIP_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cloudini_hip.h"
#include "crc32_combine.h"
#include "decode_workspace.h"
#include "encode_workspace.h"
#include "stage1_device.h"
#include "stage1_launch.h"

using namespace cldn;

namespace {

thread_local std::string g_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}

// ST_PALETTE_FULL (pal32_slow_first, section_palette): no stream was produced
constexpr const char* kPaletteFullMessage =
    "Palette section: too many distinct values share one hash partition at the largest partition count; encode this cloud under another mode";

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) {                                                                         \
      return fail(_e == hipErrorNoDevice ? CLDN_HIP_ERR_NO_DEVICE : CLDN_HIP_ERR_DEVICE,             \
                  "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);       \
    }                                                                                               \
  } while (0)

// Selects the codec's device for the duration of an ABI call and gives the calling thread its own device back
// (callers such as torch or a ROS node with several GPUs keep their own notion of the current device).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t enter(int device) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev == device) return hipSuccess;
    e = hipSetDevice(device);
    switched = (e == hipSuccess);
    return e;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
#define ENTER_DEVICE(dev) \
  DeviceGuard _device_guard;  \
  HIP_TRY(_device_guard.enter(dev))

int size_of_type(uint8_t t) {  // include/cloudini_lib/basic_types.hpp:73-95
  switch (t) {
    case 1: case 2: return 1;
    case 3: case 4: return 2;
    case 5: case 6: case 7: return 4;
    case 8: case 9: case 10: return 8;
    default: return 0;
  }
}
bool is_adaptive_int(uint8_t t) {  // src/v5_codec.cpp:83-95
  return t == 3 || t == 4 || t == 5 || t == 6 || t == 9 || t == 10;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return CLDN_HIP_OK;
    if (p) {
      HIP_TRY(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    const size_t want = (bytes + 255) & ~size_t(255);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(e == hipErrorOutOfMemory ? CLDN_HIP_ERR_NOMEM : CLDN_HIP_ERR_DEVICE,
                  "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return CLDN_HIP_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // a workspace with one carve function (decode_workspace.h): sized by its run over NULL, carved where it then lies
  template <class CarveFn>
  int ensure_carved(CarveFn carve) {
    const int rc = ensure(carve((void*)nullptr));
    if (rc == CLDN_HIP_OK) carve(p);
    return rc;
  }
};

struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return CLDN_HIP_OK;
    if (p) {
      HIP_TRY(hipHostFree(p));
      p = nullptr;
      cap = 0;
    }
    const size_t want = (bytes + 4095) & ~size_t(4095);
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return CLDN_HIP_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace

namespace cldn {
int launch_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorNoDevice ? CLDN_HIP_ERR_NO_DEVICE : CLDN_HIP_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
}
}  // namespace cldn

// The multiplier and the decoder's factor of a lossy float op for one resolution: what the plan builder puts into its ops and what
// the sweep (sweep_kernels.hip) puts into its ladders. kind: OP_QF32 (FieldEncoderFloatN_Lossy, field_encoder.cpp:24-40),
// OP_LOSSY_F32 / OP_LOSSY_F64 (FieldEncoderFloat_Lossy<T>, field_encoder.hpp:101-102).
static void lossy_float_scale(uint32_t kind, float resolution, DevOp* op) {
  if (kind == OP_QF32) {
    op->mult_f = 1.0F / resolution;
    op->res_f = resolution;
  } else if (kind == OP_LOSSY_F32) {
    op->mult_f = (float)(1.0 / (double)resolution);
    op->res_f = resolution;
  } else {
    op->mult_d = 1.0 / (double)resolution;
    op->res_d = (double)resolution;
  }
}

struct cldn_hip_plan {
  DevPlan dev;
  std::vector<cldn_hip_field_t> fields;
  uint32_t point_step = 0;
  uint8_t version = 0;
  uint8_t encoding_opt = 0;
  bool uses_v5 = false;
  uint32_t ref_max_point_bytes = 0;  // detail::MaxSerializedPointSize
  bool has_padding = false;          // some byte of a point is not covered by any field
  uint32_t floatn_lanes = 0;         // LeadingLossyFloatFieldCount: the first 3 or 4 fields form the FloatN group, else 0
  // WIDE route (stage1_wide.h): the schema does not fit the launch-argument plan (more than kMaxOps regular tokens,
  // kMaxAdaptive adaptive fields or kMaxPointStep bytes per point). `dev` then keeps only its scalar members (n_ops,
  // n_adaptive and n_gorilla are 0: nothing on the host walks its arrays), the entries are here
  bool wide = false;
  std::vector<DevOp> ops_all;
  std::vector<uint32_t> op_aux;          // OP_GORILLA64: index of the op's token buffer
  std::vector<DevAdaptive> adaptive_all;
  std::vector<uint32_t> adaptive_field;  // index of each adaptive field among the schema's fields
  uint32_t n_gorilla_all = 0;
  uint32_t n_adaptive_total() const { return wide ? (uint32_t)adaptive_all.size() : dev.n_adaptive; }
};

struct cldn_hip_codec {
  cldn_hip_plan plan;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // workspace (grow-only)
  DevBuf d_in, d_out, d_slots, d_chunks, d_cloud_first, d_payload, d_dst, d_offsets, d_modes;
  // zeroed once per encode call (by a memset, or by the piece kernel where it is the call's first launch):
  // [status block 256 B | k_finish anchors | section-handled flags | segment table]
  DevBuf d_status;
  DevBuf d_cols[kMaxAdaptive];
  DevBuf d_ranks[kMaxAdaptive];
  DevBuf d_dec_meta, d_pre_ptrs;
  DevBuf d_dec_cols[8];       // decode: dense columns of the adaptive fields that the point kernel takes its integer fields from
  // stage 2 on the device (cldn_hip_codec_set_stage2): the stage-1 streams stay in d_s1, the LZ4 blocks go straight into the output
  // chunk table of the last cldn_hip_encode_stage1_chunks call (cldn_hip_frame_chunks frames it)
  bool ct_valid = false;
  uint32_t ct_n_chunks = 0, ct_n_clouds = 0, ct_segs_per_chunk = 0;
  uint64_t ct_slot_stride = 0, ct_need = 0;
  size_t ct_segs_off = 0, ct_anchor_off = 0;
  int stage2 = 0;
  DevBuf d_s1, d_s1_offsets, d_lz_matches, d_stage2_ws, d_payload2, d_dst2, d_dec_split;
  // LZ4 blocks back into bytes (cldn_hip_decode_lz4 / cldn_hip_lz4_decompress): one worst-case slot per chunk, the offset tables
  DevBuf d_lzd_slots, d_lzd_tables;
  DevBuf d_zsd_ws;  // ZSTD decode (zstd_decode.hip): block records, weights, frame tables
  DevBuf d_s2_gather;  // cldn_hip_decode_lz4_gather / _zstd_gather: [expanded sizes u32 | verdicts u32] per chunk
  DevBuf d_finrec;            // k_finish look-back records (rec, rec2), cleared only when (re)allocated
  int decode_fill = CLDN_HIP_FILL_KEEP;  // cldn_hip_codec_set_decode_fill
  int zstd_sequences = 0;                // cldn_hip_codec_set_zstd_sequences
  int zstd_matches = 0;                  // cldn_hip_codec_set_zstd_matches
  DevBuf d_zs_seq;                       // ... its workspace (ZstdSeqLaunch); the match lists are d_lz_matches
  DevBuf d_dec_bits;          // k_mark_token_ends: token-end bitmap of the streams of a decode call
  DevBuf d_dec_secs;          // k_section_offsets: per (field, chunk) section records + per-chunk counters
  DevBuf d_dec_rec;           // k_sections_cols_fast slice records, tagged with dec_epoch, cleared only when (re)allocated
  uint32_t dec_epoch = 0;
  uint32_t finish_epoch = 0;  // tag of this call's records
  bool force_ticket = false;      // k_finish waited in vain once (ST_FINISH_TIMEOUT): from then on its workgroups take tickets
  bool test_timeout_once = false; // cldn_hip_debug_finish_timeout_once: the next encode call's first attempt reports the timeout
  uint32_t test_split_parts = 0;  // cldn_hip_debug_decode_split: 0 = by the batch's size, 1 = chained launch, 2..16 = workgroups per chunk
  uint32_t finish_retries = 0;    // calls redone through the ticket path
  DevBuf d_pieces;  // piece table of the piece kernel (stage1_fused.h)
  uint32_t n_pieces = 0;
  uint32_t last_piece_pts = 0;
  bool last_quad_major = false;
  uint64_t pending_total = 0;  // bytes of a deferred host output waiting in d_out (cldn_hip_codec_fetch_output)
  int pipeline = 0;           // cldn_hip_codec_pipeline: 0 auto, 1 generic kernel + slots, 2 piece kernel + slots
  // applyVizLossyPreprocessing workspace (viz_filter_batch): group tables, slot per point, block counts, keep bits, the
  // cloud / block tables of the batch, survivors per cloud; d_viz_out: the survivors of a fused filter + encode call
  DevBuf d_viz_keys, d_viz_slot, d_viz_blocks, d_viz_bits, d_viz_tables, d_viz_kept, d_viz_out;
  PinnedBuf h_viz;                // upload of the cloud / block tables, readback of the counts
  uint64_t viz_group_slots = 0;   // cldn_hip_debug_viz_group_slots: 0 = kVizGroupSlots
  uint32_t hist_walk = 0;         // cldn_hip_debug_hist_walk: 0 = kHistWalkBlocks
  DevBuf d_pre[kMaxGorilla];
  // WIDE route: the plan's arrays in device memory (uploaded by cldn_hip_codec_create), per-chunk scratch of the encoder,
  // per-op state of the serial decoder, Gorilla token buffers
  DevBuf d_wide_plan, d_wide_scratch, d_wide_state;
  std::vector<DevBuf> d_wide_pre;
  WidePlan wide_desc = {};
  PinnedBuf h_stage;   // chunk table upload
  // decode table upload: a ring of staging buffers, each guarded by the event recorded behind its copy, so that a call
  // does not have to drain the stream before it fills the next one
  static constexpr int kDecStageRing = 4;
  PinnedBuf h_dec_stage[kDecStageRing];
  hipEvent_t dec_stage_ev[kDecStageRing] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t dec_stage_next = 0;
  PinnedBuf h_result;  // offsets / status readback
  PinnedBuf h_modes;   // forced modes upload
  // modes of the previous encode call, copied back asynchronously: launch hint for the section kernels
  PinnedBuf h_last_modes;
  hipEvent_t ev_last_modes = nullptr;
  size_t last_modes_count = 0;  // n_clouds * n_adaptive of the copy in flight (0 = none)
  uint32_t last_modes_fields = 0;
  uint8_t hint_cache[kMaxAdaptive];  // modes seen by the most recent call whose copy has landed
  bool hint_valid = false;
  // cached batch shape
  std::vector<uint64_t> last_cloud_points;
  uint32_t last_n_chunks = 0;
  // timing
  std::vector<hipEvent_t> events;  // 5 per timing slot
  // decode: the route counters of an earlier call, copied back asynchronously (like the encoder's mode hint): when every chunk's
  // section was a small Palette the point kernel found by itself, the next call does not launch the section pre-kernels
  PinnedBuf h_dec_stats;
  hipEvent_t ev_dec_stats = nullptr;
  uint32_t dec_stats_chunks = 0;     // chunks of the call whose copy is in flight (0 = none)
  bool dec_palette_hint = false;
  bool dec_stats_seen = false;       // one copy of the counters has landed
  uint32_t dec_dv_hint = 0;          // 1: the last counters showed no DeltaVarint section decoded by k_section_dv_w, 2: every chunk's (stage1_launch.h)
  uint32_t dec_call_index = 0;
  // cldn_hip_debug_decode_trace: the per-chunk arrays of the last decode call (inside d_dec_meta)
  struct DecTrace {
    uint32_t n_chunks = 0;
    const void* meta = nullptr;  // d_dec_meta.p of that call: a later call may have moved the workspace
    const uint32_t *reg_end = nullptr, *reg_end_pre = nullptr, *slices_done = nullptr;
    const uint8_t *sec_done = nullptr, *sec_cols = nullptr;
  } dec_trace;
  hipEvent_t dec_events[4] = {nullptr, nullptr, nullptr, nullptr};  // the last decode call's (timing enabled)
  bool dec_events_valid = false;
  std::vector<uint8_t> slot_valid;
  uint64_t call_index = 0;
  // modes committed elsewhere (continuation of a cloud from a chunk boundary); empty = probe
  std::vector<uint8_t> forced_modes;
  // cldn_hip_codec_force_modes_per_cloud: [forced_clouds * adaptive fields], one row per cloud; the two setters replace each other
  std::vector<uint8_t> forced_cloud_modes;
  uint32_t forced_clouds = 0;
  // audit (audit_kernels.hip): d_audit takes host buffers of an audit call and the decode of an audited stream, d_audit_tab the
  // cloud / block / field tables, d_audit_rep the report of a call with a HOST report
  DevBuf d_audit, d_audit_tab, d_audit_rep;
  PinnedBuf h_audit;              // upload of the tables, guarded by ev_audit
  hipEvent_t ev_audit = nullptr;
  // what cldn_hip_audit_last_encode audits: where the last encode call's points and streams lie on the device
  struct LastEncode {
    bool valid = false;
    bool await_frame = false;        // cldn_hip_encode_stage1_chunks: complete once cldn_hip_frame_chunks has run
    const uint8_t* points = nullptr;
    const uint8_t* streams = nullptr;
    const uint64_t* d_offsets = nullptr;  // device [n_clouds + 1], read back when `offsets` is empty
    std::vector<uint64_t> offsets;        // host copy (calls with host outputs have read them anyway)
    std::vector<uint64_t> cloud_points;
    int kind = CLDN_HIP_STAGE2_NONE;
    const uint8_t* s1_streams = nullptr;      // kind != CLDN_HIP_STAGE2_NONE: the framed stage-1 streams behind the blocks / frames
    const uint64_t* d_s1_offsets = nullptr;   // ... and their offsets, device [n_clouds + 1]
    void drop() { valid = await_frame = false; }
  } enc;
};

// The decode calls' staging ring, first step: the next slot of h_dec_stage, with room for `bytes`, once its last upload has left it
static int dec_stage_take(cldn_hip_codec* c, size_t bytes, uint32_t* slot, void** host) {
  *slot = c->dec_stage_next++ % (uint32_t)cldn_hip_codec::kDecStageRing;
  if (c->dec_stage_ev[*slot]) HIP_TRY(hipEventSynchronize(c->dec_stage_ev[*slot]));
  else HIP_TRY(hipEventCreateWithFlags(&c->dec_stage_ev[*slot], hipEventDisableTiming));
  const int rc = c->h_dec_stage[*slot].ensure(bytes);
  *host = c->h_dec_stage[*slot].p;
  return rc;
}
// ... second step: the slot's first `bytes` go to `dst` on the codec's stream, and the slot's event is recorded behind the copy
static int dec_stage_send(cldn_hip_codec* c, uint32_t slot, void* dst, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, c->h_dec_stage[slot].p, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->dec_stage_ev[slot], c->stream));
  return CLDN_HIP_OK;
}

extern "C" {

const char* cldn_hip_last_error(void) { return g_error.c_str(); }
int cldn_hip_abi_version(void) { return CLDN_HIP_ABI_VERSION; }

int cldn_hip_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice) return 0;
  if (e != hipSuccess) return fail(CLDN_HIP_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

void* cldn_hip_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {  // page-locked for every device
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void cldn_hip_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int cldn_hip_current_device(void) {
  int d = -1;
  hipError_t e = hipGetDevice(&d);
  if (e != hipSuccess)
    return fail(e == hipErrorNoDevice ? CLDN_HIP_ERR_NO_DEVICE : CLDN_HIP_ERR_DEVICE, "hipGetDevice: %s", hipGetErrorString(e));
  return d;
}

int cldn_hip_set_current_device(int device) {
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess)
    return fail(e == hipErrorNoDevice ? CLDN_HIP_ERR_NO_DEVICE : CLDN_HIP_ERR_DEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  return CLDN_HIP_OK;
}

int cldn_hip_plan_create(const cldn_hip_field_t* fields, uint32_t n_fields, uint32_t point_step, uint8_t version,
                         uint8_t encoding_opt, cldn_hip_plan_t** out) {
  if (!out) return fail(CLDN_HIP_ERR_ARG, "plan_create: out is NULL");
  *out = nullptr;
  if (point_step == 0) return fail(CLDN_HIP_ERR_ARG, "point_step cannot be 0");  // cloudini.cpp:250-252
  if (n_fields && !fields) return fail(CLDN_HIP_ERR_ARG, "fields is NULL");
  if (encoding_opt > 2) return fail(CLDN_HIP_ERR_ARG, "invalid encoding_opt %u", encoding_opt);

  cldn_hip_plan* plan = new (std::nothrow) cldn_hip_plan();
  if (!plan) return fail(CLDN_HIP_ERR_NOMEM, "out of memory");
  plan->fields.assign(fields, fields + n_fields);
  plan->point_step = point_step;
  plan->version = version;
  plan->encoding_opt = encoding_opt;
  DevPlan& d = plan->dev;
  memset(&d, 0, sizeof(d));
  d.point_step = point_step;
  const bool lossy = encoding_opt == 1;

  // MaxSerializedPointSize (codec_common.cpp:29-67) -- also validates the field types
  for (uint32_t i = 0; i < n_fields; ++i) {
    const cldn_hip_field_t& f = fields[i];
    const int sz = size_of_type(f.type);
    if (sz == 0) {
      delete plan;
      return fail(CLDN_HIP_ERR_ARG, "Unsupported field type %u (field %u)", f.type, i);
    }
    if ((uint64_t)f.offset + (uint64_t)sz > point_step) {
      delete plan;
      return fail(CLDN_HIP_ERR_ARG, "field %u (offset %u, %d bytes) exceeds point_step %u", i, f.offset, sz,
                  point_step);
    }
    switch (f.type) {
      case 7: plan->ref_max_point_bytes += (lossy && f.has_resolution) ? 10 : 7; break;
      case 8: plan->ref_max_point_bytes += (lossy && f.has_resolution) ? 10 : 11; break;
      case 1: case 2: plan->ref_max_point_bytes += 1; break;
      default: plan->ref_max_point_bytes += 10; break;
    }
  }

  {
    std::vector<uint8_t> covered(point_step, 0);
    for (uint32_t i = 0; i < n_fields; ++i)
      for (int b = 0; b < size_of_type(fields[i].type); ++b) covered[fields[i].offset + b] = 1;
    plan->has_padding = std::find(covered.begin(), covered.end(), 0) != covered.end();
  }
  // LeadingLossyFloatFieldCount (codec_common.cpp:69-82)
  uint32_t lead = 0;
  if (lossy) {
    for (uint32_t i = 0; i < n_fields; ++i) {
      if (fields[i].type != 7 || !fields[i].has_resolution) break;
      ++lead;
    }
    if (lead != 3 && lead != 4) lead = 0;
  }
  plan->floatn_lanes = lead;
  // UsesV5Codec (v5_codec.cpp:883-892)
  plan->uses_v5 = false;
  if (version >= 5 && lossy) {
    for (uint32_t i = lead; i < n_fields; ++i) plan->uses_v5 |= is_adaptive_int(fields[i].type);
  }

  // (every op and adaptive field goes to the plan's vectors first; they move into `d`'s arrays at the end if they fit)
  auto add_op = [&](DevOp op) -> int {
    plan->ops_all.push_back(op);
    plan->op_aux.push_back(op.kind == OP_GORILLA64 ? plan->n_gorilla_all++ : 0u);
    d.max_regular_bytes += op.max_bytes;
    return CLDN_HIP_OK;
  };
  int rc = CLDN_HIP_OK;
  d.all_varint = 1;
  for (uint32_t i = 0; i < n_fields && rc == CLDN_HIP_OK; ++i) {
    const cldn_hip_field_t& f = fields[i];
    DevOp op;
    memset(&op, 0, sizeof(op));
    op.offset = f.offset;
    op.type = f.type;
    op.size = (uint8_t)size_of_type(f.type);
    if (encoding_opt == 0) {  // BuildV4Encoders, v4_codec.cpp:29-34: everything is a raw copy
      op.kind = OP_COPY;
      op.max_bytes = op.size;
      d.all_varint = 0;
      d.min_regular_bytes += op.size;
      rc = add_op(op);
      continue;
    }
    if (i < lead) {  // FieldEncoderFloatN_Lossy lane, field_encoder.cpp:24-40
      op.kind = OP_QF32;
      lossy_float_scale(OP_QF32, f.resolution, &op);
      op.max_bytes = 5;
      if (!(op.mult_f > 0.0f)) {
        rc = fail(CLDN_HIP_ERR_ARG, "FieldEncoderFloatN_Lossy requires a resolution with value > 0.0");
        break;
      }
      d.min_regular_bytes += 1;
      rc = add_op(op);
      continue;
    }
    if (plan->uses_v5 && is_adaptive_int(f.type)) {  // buildV5Plan, v5_codec.cpp:725-737
      DevAdaptive a;
      memset(&a, 0, sizeof(a));
      a.offset = f.offset;
      a.type = f.type;
      a.bpv = op.size;
      plan->adaptive_all.push_back(a);
      plan->adaptive_field.push_back(i);
      continue;
    }
    switch (f.type) {  // CreateCompatibleEncoder, codec_common.cpp:116-153
      case 7:
        if (lossy && f.has_resolution) {
          if (!(f.resolution > 0.0f)) {
            rc = fail(CLDN_HIP_ERR_ARG, "FieldEncoder(Float/Lossy) requires a resolution with value > 0.0");
            break;
          }
          op.kind = OP_LOSSY_F32;
          lossy_float_scale(OP_LOSSY_F32, f.resolution, &op);
          op.max_bytes = 10;
          d.min_regular_bytes += 1;
        } else if (encoding_opt == 2) {
          op.kind = OP_XOR32;
          op.max_bytes = 4;
          d.all_varint = 0;
          d.min_regular_bytes += 4;
        } else {
          op.kind = OP_COPY;
          op.max_bytes = 4;
          d.all_varint = 0;
          d.min_regular_bytes += 4;
        }
        break;
      case 8:
        if (lossy && f.has_resolution) {
          if (!(f.resolution > 0.0f)) {
            rc = fail(CLDN_HIP_ERR_ARG, "FieldEncoder(Float/Lossy) requires a resolution with value > 0.0");
            break;
          }
          op.kind = OP_LOSSY_F64;
          lossy_float_scale(OP_LOSSY_F64, f.resolution, &op);
          op.max_bytes = 10;
          d.min_regular_bytes += 1;
        } else if (!f.has_resolution && version >= 4) {
          op.kind = OP_GORILLA64;  // FieldEncoderFloat_Gorilla<double>
          op.type = (uint8_t)(plan->n_gorilla_all & 0xffu);  // index of the op's token buffer (the WIDE route reads op_aux instead)
          op.max_bytes = 10;       // 1 + 1 + 5 + 6 + 64 = 77 bits
          d.all_varint = 0;
          d.min_regular_bytes += 1;
        } else {
          op.kind = OP_XOR64;
          op.max_bytes = 8;
          d.all_varint = 0;
          d.min_regular_bytes += 8;
        }
        break;
      case 1: case 2:
        op.kind = OP_COPY;
        op.max_bytes = 1;
        d.all_varint = 0;
        d.min_regular_bytes += 1;
        break;
      default:
        op.kind = OP_INT;
        op.max_bytes = 10;
        d.min_regular_bytes += 1;
        break;
    }
    if (rc == CLDN_HIP_OK) rc = add_op(op);
  }
  if (rc != CLDN_HIP_OK) {
    delete plan;
    return rc;
  }
  plan->wide = plan->ops_all.size() > (size_t)kMaxOps || plan->adaptive_all.size() > (size_t)kMaxAdaptive ||
               plan->n_gorilla_all > (uint32_t)kMaxGorilla || point_step > kMaxPointStep;
  if (!plan->wide) {
    d.n_ops = (uint32_t)plan->ops_all.size();
    for (uint32_t k = 0; k < d.n_ops; ++k) d.ops[k] = plan->ops_all[k];
    d.n_adaptive = (uint32_t)plan->adaptive_all.size();
    for (uint32_t a = 0; a < d.n_adaptive; ++a) d.adaptive[a] = plan->adaptive_all[a];
    d.n_gorilla = plan->n_gorilla_all;
  } else {
    d.all_varint = 0;  // (no kernel of the ordinary route may take this plan)
  }
  {  // decode: can the token ends of the regular stream be laid out from the point's form (k_mark_token_ends)?
    bool ok = d.n_ops >= 1u && d.n_ops <= 8u && d.max_regular_bytes <= 256u;
    uint32_t n_raw = 0u;
    for (uint32_t o = 0; o < d.n_ops && ok; ++o) {
      const uint32_t k = d.ops[o].kind;
      if (k == OP_COPY || k == OP_XOR32 || k == OP_XOR64) {
        const uint32_t sz = d.ops[o].size;
        ok = sz == 1u || sz == 2u || sz == 4u || sz == 8u;
        ++n_raw;
      } else {
        ok = k == OP_QF32 || k == OP_LOSSY_F32 || k == OP_LOSSY_F64 || k == OP_INT;
      }
    }
    d.varint_and_raw = (ok && n_raw != 0u) ? 1u : 0u;
  }
  *out = plan;
  return CLDN_HIP_OK;
}

void cldn_hip_plan_destroy(cldn_hip_plan_t* plan) { delete plan; }
int cldn_hip_plan_uses_v5(const cldn_hip_plan_t* plan) { return plan && plan->uses_v5 ? 1 : 0; }
uint32_t cldn_hip_plan_adaptive_fields(const cldn_hip_plan_t* plan) { return plan ? plan->n_adaptive_total() : 0; }
uint32_t cldn_hip_plan_adaptive_field_index(const cldn_hip_plan_t* plan, uint32_t a) {
  return plan && a < plan->adaptive_field.size() ? plan->adaptive_field[a] : 0xffffffffu;
}
uint32_t cldn_hip_plan_max_point_bytes(const cldn_hip_plan_t* plan) { return plan ? plan->ref_max_point_bytes : 0; }

uint64_t cldn_hip_stage1_bound(const cldn_hip_plan_t* plan, uint64_t n_points) {  // cloudini.cpp:249-292 (NONE)
  if (!plan) return 0;
  uint64_t total = 0, left = n_points;
  while (left > 0) {
    const uint64_t in_chunk = std::min<uint64_t>(left, kPointsPerChunk);
    left -= in_chunk;
    uint64_t chunk = in_chunk * plan->ref_max_point_bytes;
    if (plan->uses_v5) chunk += (uint64_t)plan->fields.size() * 32u + 1024u;
    total += 4 + chunk;
  }
  return total;
}

static uint64_t lz4_block_bound(uint64_t n) { return n + n / 255u + 16u; }  // LZ4_COMPRESSBOUND, lz4.h
// ZSTD_COMPRESSBOUND, zstd.h (what MaxCompressedSize uses). A frame of zstd_kernels.hip never exceeds it: 9 bytes of frame
// header and 3 per 128 KiB block over the payload
static uint64_t zstd_frame_bound(uint64_t n) { return n + (n >> 8) + (n < 131072u ? (131072u - n) >> 11 : 0u); }

uint64_t cldn_hip_stage2_bound(const cldn_hip_plan_t* plan, uint64_t n_points, int stage2) {  // cloudini.cpp:249-292
  if (!plan) return 0;
  if (stage2 == CLDN_HIP_STAGE2_NONE) return cldn_hip_stage1_bound(plan, n_points);
  uint64_t total = 0, left = n_points;
  while (left > 0) {
    const uint64_t in_chunk = std::min<uint64_t>(left, kPointsPerChunk);
    left -= in_chunk;
    uint64_t chunk = in_chunk * plan->ref_max_point_bytes;
    if (plan->uses_v5) chunk += (uint64_t)plan->fields.size() * 32u + 1024u;
    total += 4 + (stage2 == CLDN_HIP_STAGE2_ZSTD ? zstd_frame_bound(chunk) : lz4_block_bound(chunk));
  }
  return total;
}

int cldn_hip_codec_set_stage2(cldn_hip_codec_t* c, int stage2) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (stage2 != CLDN_HIP_STAGE2_NONE && stage2 != CLDN_HIP_STAGE2_LZ4 && stage2 != CLDN_HIP_STAGE2_LZ4_FAST &&
      stage2 != CLDN_HIP_STAGE2_ZSTD)
    return fail(CLDN_HIP_ERR_ARG, "invalid stage-2 mode %d", stage2);
  c->stage2 = stage2;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_create(const cldn_hip_plan_t* plan, int device, void* hip_stream, cldn_hip_codec_t** out) {
  if (!plan || !out) return fail(CLDN_HIP_ERR_ARG, "codec_create: NULL argument");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(CLDN_HIP_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                hipGetErrorString(e));
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= n) return fail(CLDN_HIP_ERR_ARG, "device %d out of range (%d devices)", device, n);
  ENTER_DEVICE(device);
  cldn_hip_codec* c = new (std::nothrow) cldn_hip_codec();
  if (!c) return fail(CLDN_HIP_ERR_NOMEM, "out of memory");
  c->plan = *plan;
  c->device = device;
  if (hip_stream) {
    c->stream = (hipStream_t)hip_stream;
  } else {
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
      delete c;
      return fail(CLDN_HIP_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(se));
    }
    c->own_stream = true;
  }
  int rc = stage1_configure_kernels();
  if (rc == CLDN_HIP_OK) rc = lz4_configure_decode();
  if (rc == CLDN_HIP_OK) rc = modes_configure();
  if (rc == CLDN_HIP_OK && c->plan.wide) {
    // WIDE route: [ops | op_aux | adaptive] in one device buffer, the descriptor that points into it
    const cldn_hip_plan& P = c->plan;
    const size_t ops_b = (P.ops_all.size() * sizeof(DevOp) + 63u) & ~size_t(63);
    const size_t aux_b = (P.op_aux.size() * sizeof(uint32_t) + 63u) & ~size_t(63);
    const size_t ada_b = (P.adaptive_all.size() * sizeof(DevAdaptive) + 63u) & ~size_t(63);
    rc = c->d_wide_plan.ensure(ops_b + aux_b + ada_b + 64u);
    if (rc == CLDN_HIP_OK) {
      uint8_t* base = (uint8_t*)c->d_wide_plan.p;
      hipError_t he = hipSuccess;
      if (!P.ops_all.empty()) he = hipMemcpy(base, P.ops_all.data(), P.ops_all.size() * sizeof(DevOp), hipMemcpyHostToDevice);
      if (he == hipSuccess && !P.op_aux.empty())
        he = hipMemcpy(base + ops_b, P.op_aux.data(), P.op_aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
      if (he == hipSuccess && !P.adaptive_all.empty())
        he = hipMemcpy(base + ops_b + aux_b, P.adaptive_all.data(), P.adaptive_all.size() * sizeof(DevAdaptive), hipMemcpyHostToDevice);
      if (he != hipSuccess) rc = fail(CLDN_HIP_ERR_DEVICE, "upload of the wide plan: %s", hipGetErrorString(he));
      WidePlan& W = c->wide_desc;
      W.point_step = P.point_step;
      W.n_ops = (uint32_t)P.ops_all.size();
      W.n_adaptive = (uint32_t)P.adaptive_all.size();
      W.n_gorilla = P.n_gorilla_all;
      W.min_regular_bytes = P.dev.min_regular_bytes;
      W.reserved = 0u;
      W.ops = reinterpret_cast<const DevOp*>(base);
      W.op_aux = reinterpret_cast<const uint32_t*>(base + ops_b);
      W.adaptive = reinterpret_cast<const DevAdaptive*>(base + ops_b + aux_b);
      c->d_wide_pre.resize(P.n_gorilla_all);
    }
  }
  if (rc != CLDN_HIP_OK) {
    cldn_hip_codec_destroy(c);
    return rc;
  }
  *out = c;
  return CLDN_HIP_OK;
}

void cldn_hip_codec_destroy(cldn_hip_codec_t* c) {
  if (!c) return;
  DeviceGuard guard;
  (void)guard.enter(c->device);
  (void)hipStreamSynchronize(c->stream);
  DevBuf* bufs[] = {&c->d_in, &c->d_out, &c->d_slots, &c->d_chunks, &c->d_cloud_first, &c->d_finrec, &c->d_dec_rec, &c->d_dec_bits, &c->d_dec_secs, &c->d_s1, &c->d_s1_offsets,
                    &c->d_lz_matches, &c->d_zs_seq, &c->d_stage2_ws, &c->d_payload2, &c->d_dst2, &c->d_dec_split, &c->d_lzd_slots, &c->d_lzd_tables, &c->d_zsd_ws, &c->d_s2_gather,
                    &c->d_payload, &c->d_dst, &c->d_offsets, &c->d_modes, &c->d_status, &c->d_dec_meta, &c->d_pre_ptrs, &c->d_dec_cols[0], &c->d_dec_cols[1], &c->d_dec_cols[2], &c->d_dec_cols[3], &c->d_dec_cols[4], &c->d_dec_cols[5], &c->d_dec_cols[6], &c->d_dec_cols[7],
                    &c->d_viz_keys, &c->d_viz_slot, &c->d_viz_blocks, &c->d_viz_bits, &c->d_viz_tables, &c->d_viz_kept, &c->d_viz_out,
                    &c->d_pieces, &c->d_audit, &c->d_audit_tab, &c->d_audit_rep};
  for (DevBuf* b : bufs) b->release();
  for (int a = 0; a < kMaxAdaptive; ++a) {
    c->d_cols[a].release();
    c->d_ranks[a].release();
  }
  for (int g = 0; g < kMaxGorilla; ++g) c->d_pre[g].release();
  c->d_wide_plan.release();
  c->d_wide_scratch.release();
  c->d_wide_state.release();
  for (DevBuf& b : c->d_wide_pre) b.release();
  c->h_stage.release();
  c->h_viz.release();
  c->h_audit.release();
  if (c->ev_audit) (void)hipEventDestroy(c->ev_audit);
  for (int k = 0; k < cldn_hip_codec::kDecStageRing; ++k) {
    c->h_dec_stage[k].release();
    if (c->dec_stage_ev[k]) (void)hipEventDestroy(c->dec_stage_ev[k]);
  }
  c->h_result.release();
  c->h_modes.release();
  c->h_last_modes.release();
  if (c->ev_last_modes) (void)hipEventDestroy(c->ev_last_modes);
  c->h_dec_stats.release();
  if (c->ev_dec_stats) (void)hipEventDestroy(c->ev_dec_stats);
  for (hipEvent_t& ev : c->events)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t& ev : c->dec_events)
    if (ev) (void)hipEventDestroy(ev);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int cldn_hip_codec_synchronize(cldn_hip_codec_t* c) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  HIP_TRY(hipStreamSynchronize(c->stream));
  return CLDN_HIP_OK;
}

void* cldn_hip_codec_stream(cldn_hip_codec_t* c) { return c ? (void*)c->stream : nullptr; }
int cldn_hip_codec_device(const cldn_hip_codec_t* c) { return c ? c->device : CLDN_HIP_ERR_ARG; }

int cldn_hip_codec_enable_timing(cldn_hip_codec_t* c, uint32_t n_slots) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  ENTER_DEVICE(c->device);
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (hipEvent_t& ev : c->events)
    if (ev) (void)hipEventDestroy(ev);
  c->events.assign((size_t)n_slots * 5, nullptr);
  c->slot_valid.assign(n_slots, 0);
  for (hipEvent_t& ev : c->events) HIP_TRY(hipEventCreate(&ev));
  c->call_index = 0;
  c->dec_events_valid = false;
  for (hipEvent_t& ev : c->dec_events) {
    if (n_slots && !ev) HIP_TRY(hipEventCreate(&ev));
    if (!n_slots && ev) {
      (void)hipEventDestroy(ev);
      ev = nullptr;
    }
  }
  return CLDN_HIP_OK;
}

// Test hook, outside the boundary of include/cloudini_hip.h (like cldn_hip_debug_finish_trace): the codec's next encode call
// reports ST_FINISH_TIMEOUT on its first attempt, so that the retry through the ticket order can be exercised
// (tests/test_gpu_encode.py). Rounds 3-4 read an environment variable in the encode path for this.
__attribute__((visibility("default"))) int cldn_hip_debug_finish_timeout_once(cldn_hip_codec_t* c) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->test_timeout_once = true;
  return CLDN_HIP_OK;
}

// Test hook, outside the boundary like the one above: which launch shape the point decoder takes (tests/test_gpu_decode.py
// runs every schema family through the chained and the SPLIT launches whatever the batch's size). parts: 0 = decided by the
// number of chunks (the default), 1 = the chained launch, 2..16 = a SPLIT launch with that many workgroups per chunk. Bytes
// never depend on it. (Rounds 4-5 read environment variables in the decode path for this.)
__attribute__((visibility("default"))) int cldn_hip_debug_decode_split(cldn_hip_codec_t* c, uint32_t parts) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (parts > 16u) return fail(CLDN_HIP_ERR_ARG, "at most 16 workgroups per chunk");
  c->test_split_parts = parts;
  return CLDN_HIP_OK;
}

// Test hook: the bytes of k_zstd_seq_exec's LDS ring (zstd_seq_decode.hip), for the tests that place matches at its boundary
__attribute__((visibility("default"))) uint32_t cldn_hip_debug_zstd_seq_ring(void) { return zstd_seq_ring_bytes(); }

// Test hook, outside the boundary like the ones above: what the codec's last decode call decided, read from its workspace behind a
// stream synchronise (tests/test_gpu_locate.py holds it against tests/locate_model.py). words: the decode counters (kStatFastRegular
// .. kStatDvGuess, status_block.h). Per chunk, `capacity` entries each (any may be NULL): reg_end_pre / slices_done / sec_cols as the
// kernels in front of the point kernel left them, reg_end / sec_done as the call left them. Arrays no kernel of the call's route
// writes hold stale bytes, and any later call of the codec reuses the status block: ask straight after the decode call.
// *n_chunks: chunks of that call (0: no decode call yet); more than `capacity` is an error.
__attribute__((visibility("default"))) int cldn_hip_debug_decode_trace(cldn_hip_codec_t* c, uint32_t words[8], uint32_t capacity,
                                                                       uint32_t* n_chunks, uint32_t* reg_end_pre, uint32_t* slices_done,
                                                                       uint8_t* sec_cols, uint32_t* reg_end, uint8_t* sec_done) {
  if (!c || !words || !n_chunks) return fail(CLDN_HIP_ERR_ARG, "decode_trace: NULL argument");
  memset(words, 0, kStatCount * sizeof(uint32_t));
  const cldn_hip_codec::DecTrace& t = c->dec_trace;
  *n_chunks = t.n_chunks;
  if (!c->d_status.p) return CLDN_HIP_OK;
  if (t.n_chunks && t.meta != c->d_dec_meta.p) return fail(CLDN_HIP_ERR_ARG, "decode_trace: the last decode call's workspace is gone");
  if (t.n_chunks > capacity) return fail(CLDN_HIP_ERR_CAPACITY, "decode_trace: %u chunks, room for %u", t.n_chunks, capacity);
  ENTER_DEVICE(c->device);
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(words, (const uint32_t*)c->d_status.p + kStatFirst, kStatCount * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t n = t.n_chunks;
  if (n && reg_end_pre) HIP_TRY(hipMemcpy(reg_end_pre, t.reg_end_pre, n * 4u, hipMemcpyDeviceToHost));
  if (n && slices_done) HIP_TRY(hipMemcpy(slices_done, t.slices_done, n * 4u, hipMemcpyDeviceToHost));
  if (n && sec_cols) HIP_TRY(hipMemcpy(sec_cols, t.sec_cols, n, hipMemcpyDeviceToHost));
  if (n && reg_end) HIP_TRY(hipMemcpy(reg_end, t.reg_end, n * 4u, hipMemcpyDeviceToHost));
  if (n && sec_done) HIP_TRY(hipMemcpy(sec_done, t.sec_done, n, hipMemcpyDeviceToHost));
  return CLDN_HIP_OK;
}

// Test hook, outside the boundary like the ones above: the table slots a cloud group of the viz pre-filter may take
// (0 = CLDN_HIP_VIZ_GROUP_SLOTS). A cloud whose table alone is larger forms a group of its own, so 1 puts every cloud into its
// own group (tests/test_viz_batch.py). Bytes never depend on it.
__attribute__((visibility("default"))) int cldn_hip_debug_viz_group_slots(cldn_hip_codec_t* c, uint64_t slots) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->viz_group_slots = slots;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_decode_ms(cldn_hip_codec_t* c, float ms[2]) {
  if (!c || !ms) return fail(CLDN_HIP_ERR_ARG, "NULL argument");
  if (!c->dec_events_valid) return fail(CLDN_HIP_ERR_ARG, "no timed decode call (cldn_hip_codec_enable_timing first)");
  HIP_TRY(hipEventSynchronize(c->dec_events[3]));
  HIP_TRY(hipEventElapsedTime(&ms[0], c->dec_events[1], c->dec_events[2]));
  HIP_TRY(hipEventElapsedTime(&ms[1], c->dec_events[0], c->dec_events[3]));
  return CLDN_HIP_OK;
}

int cldn_hip_codec_kernel_ms(cldn_hip_codec_t* c, uint32_t slot, float ms[4]) {
  if (!c || !ms) return fail(CLDN_HIP_ERR_ARG, "NULL argument");
  if (slot >= c->slot_valid.size() || !c->slot_valid[slot]) return fail(CLDN_HIP_ERR_ARG, "no timed call in slot %u", slot);
  hipEvent_t* ev = &c->events[(size_t)slot * 5];
  HIP_TRY(hipEventSynchronize(ev[4]));
  HIP_TRY(hipEventElapsedTime(&ms[3], ev[0], ev[4]));
  HIP_TRY(hipEventElapsedTime(&ms[0], ev[1], ev[2]));
  HIP_TRY(hipEventElapsedTime(&ms[1], ev[2], ev[3]));
  HIP_TRY(hipEventElapsedTime(&ms[2], ev[3], ev[4]));
  return CLDN_HIP_OK;
}

int cldn_hip_codec_status(cldn_hip_codec_t* c) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  ENTER_DEVICE(c->device);
  if (!c->d_status.p) return CLDN_HIP_OK;
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->d_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st & ST_FINISH_TIMEOUT) {
    c->force_ticket = true;  // (device-resident outputs cannot be redone here: the caller repeats the call, which then takes tickets)
    return fail(CLDN_HIP_ERR_DEVICE, "k_finish: a workgroup waited too long for the sizes of the chunks before it (status 0x%x); the codec uses the ticket order from now on, repeat the call", st);
  }
  if (st & ST_PALETTE_FULL) return fail(CLDN_HIP_ERR_UNSUPPORTED, kPaletteFullMessage);
  if (st & ST_OUT_OVERFLOW) return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for the encoded stream");
  if (st & ST_LZ4_REJECT) return fail(CLDN_HIP_ERR_CORRUPT, "LZ4 decompression failed");
  if (st & ST_ZSTD_REJECT) return fail(CLDN_HIP_ERR_CORRUPT, "ZSTD decompression failed");
  if (st & ST_ZSTD_HOST) return fail(CLDN_HIP_ERR_UNSUPPORTED, "ZSTD frame carries sequences or options the device decoder does not take");
  if (st & ST_CORRUPT) return fail(CLDN_HIP_ERR_CORRUPT, "malformed stage-1 stream");
  return CLDN_HIP_OK;
}

// Build (or reuse) the chunk table of a batch of n_chunks chunks (the caller counted them: at most 0x3fffffff).
// piece_pts != 0: also the piece table of the single-pass encoder (pieces of piece_pts points, per chunk padded to 4)
// quad_major: the piece table lists workgroup 0 (pieces 0..3) of every chunk, then workgroup 1 of every chunk, ... so
// that the workgroups of ONE chunk start far apart in time (intra-chunk placement of the piece kernel)
static int upload_batch_shape(cldn_hip_codec* c, const uint64_t* cloud_points, uint32_t n_clouds, uint32_t n_chunks, uint32_t piece_pts,
                              bool quad_major) {
  int rc;
  const bool same = c->last_cloud_points.size() == n_clouds && c->last_n_chunks == n_chunks &&
                    c->last_piece_pts == piece_pts && c->last_quad_major == quad_major &&
                    std::equal(c->last_cloud_points.begin(), c->last_cloud_points.end(), cloud_points);
  uint64_t n_pieces64 = 0;
  if (piece_pts) {
    for (uint32_t k = 0; k < n_clouds; ++k) {
      const uint64_t full = cloud_points[k] / kPointsPerChunk, rest = cloud_points[k] % kPointsPerChunk;
      n_pieces64 += full * ((((uint64_t)kPointsPerChunk + piece_pts - 1) / piece_pts + 3) & ~uint64_t(3));
      if (rest) n_pieces64 += ((rest + piece_pts - 1) / piece_pts + 3) & ~uint64_t(3);
    }
    if (n_pieces64 > 0x7fffffffull) return fail(CLDN_HIP_ERR_ARG, "batch too large");
  }
  c->n_pieces = (uint32_t)n_pieces64;
  if (piece_pts && (rc = c->d_pieces.ensure(std::max<size_t>(1, (size_t)n_pieces64) * sizeof(PieceDesc))) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_chunks.ensure(std::max<size_t>(1, n_chunks) * sizeof(ChunkDesc))) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_cloud_first.ensure((size_t)(n_clouds + 1) * sizeof(uint32_t))) != CLDN_HIP_OK) return rc;
  if (same) return CLDN_HIP_OK;

  const size_t head_bytes = ((size_t)n_chunks * sizeof(ChunkDesc) + (size_t)(n_clouds + 1) * sizeof(uint32_t) + 31) & ~size_t(31);
  const size_t bytes = head_bytes + (size_t)n_pieces64 * sizeof(PieceDesc);
  // the staging buffer may still be in flight from the previous (asynchronous) call
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((rc = c->h_stage.ensure(bytes)) != CLDN_HIP_OK) return rc;
  ChunkDesc* hc = (ChunkDesc*)c->h_stage.p;
  uint32_t* hf = (uint32_t*)((uint8_t*)c->h_stage.p + (size_t)n_chunks * sizeof(ChunkDesc));
  uint64_t first = 0;
  uint32_t ci = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    hf[k] = ci;
    uint64_t left = cloud_points[k];
    uint32_t j = 0;
    while (left > 0) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(left, kPointsPerChunk);
      ChunkDesc& cd = hc[ci++];
      cd.first_point = first;
      cd.n_points = n;
      cd.cloud = k;
      cd.chunk_in_cloud = j++;
      cd.reserved = 0;
      first += n;
      left -= n;
    }
  }
  hf[n_clouds] = ci;
  if (piece_pts && n_pieces64) {
    PieceDesc* hp = (PieceDesc*)((uint8_t*)c->h_stage.p + head_bytes);
    size_t g = 0;
    auto put = [&](uint32_t k, uint32_t q, uint32_t P) {
      hp[g].chunk_first_point = hc[k].first_point;
      hp[g].chunk = k;
      hp[g].cloud = hc[k].cloud;
      hp[g].n_chunk_points = hc[k].n_points;
      hp[g].p = (uint16_t)q;
      hp[g].P = (uint16_t)P;
      hp[g].pad[0] = hp[g].pad[1] = 0;
      ++g;
    };
    const uint32_t max_p = (((kPointsPerChunk + piece_pts - 1) / piece_pts) + 3u) & ~3u;
    if (!quad_major) {
      for (uint32_t k = 0; k < n_chunks; ++k) {
        const uint32_t P = (((hc[k].n_points + piece_pts - 1) / piece_pts) + 3u) & ~3u;
        for (uint32_t q = 0; q < P; ++q) put(k, q, P);
      }
    } else {
      for (uint32_t q0 = 0; q0 < max_p; q0 += 4u)
        for (uint32_t k = 0; k < n_chunks; ++k) {
          const uint32_t P = (((hc[k].n_points + piece_pts - 1) / piece_pts) + 3u) & ~3u;
          if (q0 < P)
            for (uint32_t q = q0; q < q0 + 4u; ++q) put(k, q, P);
        }
    }
    HIP_TRY(hipMemcpyAsync(c->d_pieces.p, hp, g * sizeof(PieceDesc), hipMemcpyHostToDevice, c->stream));
  }
  c->last_piece_pts = piece_pts;
  c->last_quad_major = quad_major;
  if (n_chunks)
    HIP_TRY(hipMemcpyAsync(c->d_chunks.p, hc, (size_t)n_chunks * sizeof(ChunkDesc), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_cloud_first.p, hf, (size_t)(n_clouds + 1) * sizeof(uint32_t), hipMemcpyHostToDevice,
                         c->stream));
  c->last_cloud_points.assign(cloud_points, cloud_points + n_clouds);
  c->last_n_chunks = n_chunks;
  return CLDN_HIP_OK;
}

}  // extern "C"

// cloud_ptrs != NULL: the clouds live in separate HOST buffers (`points` is ignored)
// table != NULL: chunk-table output (cldn_hip_encode_stage1_chunks): no framing, `out` is not used
constexpr int kRetryWithTicket = 0x7fff0001;  // encode_stage1_once: k_finish timed out without the ticket, the call is redone with it

// host clouds (one buffer, or one per cloud) into d_in, back to back
static int stage_host_input(cldn_hip_codec* c, const void* points, const void* const* cloud_ptrs, const uint64_t* cloud_points,
                           uint32_t n_clouds, uint32_t point_step, uint64_t bytes) {
  int rc;
  if ((rc = c->d_in.ensure((size_t)bytes)) != CLDN_HIP_OK) return rc;
  if (!cloud_ptrs) {
    HIP_TRY(hipMemcpyAsync(c->d_in.p, points, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return CLDN_HIP_OK;
  }
  size_t at = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    const size_t b = (size_t)cloud_points[k] * point_step;
    if (b) HIP_TRY(hipMemcpyAsync((uint8_t*)c->d_in.p + at, cloud_ptrs[k], b, hipMemcpyHostToDevice, c->stream));
    at += b;
  }
  return CLDN_HIP_OK;
}

// How many sub-ranges the match lists of a stage-2 call are sized for (LZ4, and ZSTD with matches): every chunk has
// ceil(payload / sub-range bytes) of them. *stage1_failed: no stage 2 over stale sizes -- the stream offsets are cleared and the
// status handling of the caller (ticket retry / error) takes it from here.
static int size_match_lists(cldn_hip_codec_t* c, uint32_t n_chunks, uint32_t n_clouds, uint64_t need_s1, uint32_t lz_sub, uint32_t lz_mm,
                            uint64_t* max_subs_out, bool* stage1_failed_out) {
  uint64_t max_subs = need_s1 / lz_sub + n_chunks;
  // the match lists take as many bytes as the payloads they describe: sized from the worst-case stage-1 bound that is
  // gigabytes for a large batch (32 x 1 M XYZI points: 1.3 GB for 207 MB of payload). Beyond 256 MB the call waits for
  // stage 1 and sizes them from the bytes it really wrote (one 8-byte read; the wait is ~5 % of what the LZ4 stage takes)
  bool stage1_failed = false;
  if (max_subs * lz_mm * sizeof(LzMatch) > (256ull << 20)) {
    uint64_t total_s1 = 0;
    uint32_t st1 = 0;  // the status word travels with the total: behind a stage 1 that gave up (ST_FINISH_TIMEOUT: k_finish
                       // returned before it wrote offsets, payload sizes and positions) the total is a stale number
    HIP_TRY(hipMemcpyAsync(&total_s1, (const uint64_t*)c->d_s1_offsets.p + n_clouds, sizeof(total_s1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&st1, c->d_status.p, sizeof(st1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    stage1_failed = st1 != 0u;
    if (!stage1_failed && total_s1 <= need_s1) max_subs = total_s1 / lz_sub + n_chunks;  // (every chunk's last sub-range may be partial)
  }
  if (stage1_failed) HIP_TRY(hipMemsetAsync(c->d_offsets.p, 0, (size_t)(n_clouds + 1) * sizeof(uint64_t), c->stream));
  *max_subs_out = max_subs;
  *stage1_failed_out = stage1_failed;
  return CLDN_HIP_OK;
}

// Stage 2 on the device, behind stage1_launch_encode of a call whose codec asks for it: the chunks' stage-1 payloads in d_s1 become
// LZ4 blocks (lz4_kernels.hip) or ZSTD frames of literal-only blocks (zstd_kernels.hip), written straight into the framed streams
// at `out`, with their sizes and the clouds' stream offsets (d_offsets). *d_sizes becomes the buffer chunk_sizes reports where a
// writer ran. The payloads of the batch are bounded by need_s1, the size of d_s1.
static int launch_device_stage2(cldn_hip_codec_t* c, uint32_t n_chunks, uint32_t n_clouds, uint64_t need_s1, uint8_t* out,
                                uint64_t out_capacity, const void** d_sizes) {
  int rc;
  if (n_chunks == 0u) {
    HIP_TRY(hipMemsetAsync(c->d_offsets.p, 0, (size_t)(n_clouds + 1) * sizeof(uint64_t), c->stream));
    return CLDN_HIP_OK;
  }
  Stage2Io io;
  io.stream = c->stream;
  io.stage1 = (const uint8_t*)c->d_s1.p;
  io.stage1_capacity = need_s1;
  io.chunk_dst = (const uint64_t*)c->d_dst.p;
  io.chunk_payload = (const uint32_t*)c->d_payload.p;
  io.n_chunks = n_chunks;
  io.cloud_first_chunk = (const uint32_t*)c->d_cloud_first.p;
  io.n_clouds = n_clouds;
  io.chunk_sizes = (uint32_t*)c->d_payload2.p;
  io.stream_offsets = (uint64_t*)c->d_offsets.p;
  io.out = out;
  io.out_capacity = out_capacity;
  io.status = (uint32_t*)c->d_status.p;
  if (c->stage2 == CLDN_HIP_STAGE2_ZSTD) {
    // every chunk has ceil(payload / 128 KiB) blocks, one at least
    const uint64_t max_blocks = need_s1 / kZsBlockBytes + n_chunks;
    ZstdSeqLaunch Q;
    if (c->zstd_matches) {  // the match search of the LZ4 route with the standard parameters, its lists sized by the same rule
      uint64_t max_subs = 0;
      bool stage1_failed = false;
      if ((rc = size_match_lists(c, n_chunks, n_clouds, need_s1, kLzSubBytes, kLzMaxMatches, &max_subs, &stage1_failed)) != CLDN_HIP_OK) return rc;
      if (stage1_failed) return CLDN_HIP_OK;
      if ((rc = c->d_lz_matches.ensure((size_t)max_subs * kLzMaxMatches * sizeof(LzMatch))) != CLDN_HIP_OK) return rc;
      if ((rc = c->d_zs_seq.ensure(ZstdSeqLaunch::workspace_bytes(max_subs, max_blocks, n_chunks))) != CLDN_HIP_OK) return rc;
      Q.matches = (LzMatch*)c->d_lz_matches.p;
      Q.carve(c->d_zs_seq.p, max_subs, max_blocks, n_chunks);
    }
    if ((rc = c->d_stage2_ws.ensure(ZstdLaunch::workspace_bytes(max_blocks, n_chunks))) != CLDN_HIP_OK) return rc;
    ZstdLaunch Z;
    Z.io = io;
    Z.carve(c->d_stage2_ws.p, max_blocks, n_chunks);
    Z.seq = c->zstd_matches ? &Q : nullptr;
    if ((rc = zstd_launch(Z)) != CLDN_HIP_OK) return rc;
    *d_sizes = c->d_payload2.p;
    return CLDN_HIP_OK;
  }
  // every chunk has ceil(payload / sub-range bytes) sub-ranges
  const bool lz4_fast = c->stage2 == CLDN_HIP_STAGE2_LZ4_FAST;
  const uint32_t lz_sub = lz4_fast ? kLzFastSubBytes : kLzSubBytes, lz_mm = lz4_fast ? kLzFastMaxMatches : kLzMaxMatches;
  uint64_t max_subs = 0;
  bool stage1_failed = false;
  if ((rc = size_match_lists(c, n_chunks, n_clouds, need_s1, lz_sub, lz_mm, &max_subs, &stage1_failed)) != CLDN_HIP_OK) return rc;
  if (stage1_failed) return CLDN_HIP_OK;
  if ((rc = c->d_lz_matches.ensure((size_t)max_subs * lz_mm * sizeof(LzMatch))) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_stage2_ws.ensure(Lz4Launch::workspace_bytes(max_subs, n_chunks))) != CLDN_HIP_OK) return rc;
  Lz4Launch Z;
  Z.io = io;
  Z.fast = lz4_fast ? 1u : 0u;
  Z.matches = (LzMatch*)c->d_lz_matches.p;
  Z.block_dst = (uint64_t*)c->d_dst2.p;
  Z.carve(c->d_stage2_ws.p, max_subs, n_chunks);
  if ((rc = lz4_launch(Z)) != CLDN_HIP_OK) return rc;
  *d_sizes = c->d_payload2.p;
  return CLDN_HIP_OK;
}

static int encode_stage1_once(cldn_hip_codec_t* c, const void* points, int points_loc, const void* const* cloud_ptrs,
                              const uint64_t* cloud_points, uint32_t n_clouds, void* out, uint64_t out_capacity, int out_loc,
                              uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes,
                              cldn_hip_chunk_table_t* table = nullptr) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (table) {
    memset(table, 0, sizeof(*table));
    c->ct_valid = false;
    if (c->stage2 != CLDN_HIP_STAGE2_NONE) return fail(CLDN_HIP_ERR_ARG, "chunk-table output and stage 2 on the device exclude each other");
  }
  if (n_clouds && !cloud_points) return fail(CLDN_HIP_ERR_ARG, "cloud_points is NULL");
  if ((points_loc != CLDN_HIP_HOST && points_loc != CLDN_HIP_DEVICE) ||
      (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (c->forced_clouds && c->forced_clouds != n_clouds)
    return fail(CLDN_HIP_ERR_ARG, "modes are forced for %u clouds (cldn_hip_codec_force_modes_per_cloud), the call has %u",
                c->forced_clouds, n_clouds);
  ENTER_DEVICE(c->device);
  c->ct_valid = false;  // (the workspace is about to be rewritten)
  c->enc.drop();
  const DevPlan& plan = c->plan.dev;
  const uint32_t step = plan.point_step;

  const bool wide = c->plan.wide;  // stage1_wide.h: the plan's arrays live in device memory, one segment per chunk
  // stage 2 runs on the device (launch_device_stage2): the stage-1 streams go to d_s1, the call's output is written by the
  // stage-2 kernels. `zstd`: those are zstd_kernels.hip's, else lz4_kernels.hip's
  const bool device_stage2 = c->stage2 != CLDN_HIP_STAGE2_NONE;
  const bool zstd = c->stage2 == CLDN_HIP_STAGE2_ZSTD;
  const uint32_t n_adaptive = c->plan.n_adaptive_total();
  // capacity contract of PointcloudEncoder::encode (cloudini.cpp:531-534)
  uint64_t need = 0, need_s1 = 0, n_chunks64 = 0, n_points = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    need_s1 += cldn_hip_stage1_bound(&c->plan, cloud_points[k]);
    need += cldn_hip_stage2_bound(&c->plan, cloud_points[k], c->stage2);
    n_points += cloud_points[k];
    n_chunks64 += (cloud_points[k] + kPointsPerChunk - 1) / kPointsPerChunk;
  }
  if (n_chunks64 > 0x3fffffffull) return fail(CLDN_HIP_ERR_ARG, "batch too large");
  const uint32_t n_chunks = (uint32_t)n_chunks64;  // the route's geometry and every buffer size below rest on this one count
  // two-step host output (cldn_hip_codec_fetch_output): no caller buffer yet, the codec's own device buffer takes the bound
  const bool deferred = out == nullptr && out_loc == CLDN_HIP_HOST && !table;
  if (deferred || table) out_capacity = need;

  // The call's route (stage1_encode_route.h), once: which kernels run, and the geometry of slots and segment table that the
  // buffers below are sized from. Its facts first: the mode hints, whether the modes are forced, where the modes may go.
  // (The hint refresh used to sit behind the argument checks and the sizing. Up here a call that then fails with ARG or
  // CAPACITY has already taken the landed copy into hint_cache, and the event is queried a little earlier: the hints only
  // steer which section kernels are launched, never a byte.)
  if (!wide && c->last_modes_count && c->ev_last_modes && hipEventQuery(c->ev_last_modes) == hipSuccess) {
    // a copy of an earlier call's modes has landed: it becomes the hint until a newer one lands
    const uint8_t* lm = (const uint8_t*)c->h_last_modes.p;
    const uint32_t nf = c->last_modes_fields;
    for (uint32_t a = 0; a < (uint32_t)kMaxAdaptive; ++a) c->hint_cache[a] = 0;
    for (size_t k = 0; k < c->last_modes_count; ++k) {
      const uint8_t m = lm[k];
      c->hint_cache[k % nf] |= (m <= 3u) ? (uint8_t)(1u << m) : (uint8_t)0xF;
    }
    c->hint_valid = true;
    c->last_modes_count = 0;
  }
  EncodeFacts F = {};
  F.n_chunks = n_chunks;
  F.n_clouds = n_clouds;
  F.n_points = n_points;
  F.pipeline = (uint8_t)c->pipeline;
  F.wide = wide;
  F.chunks_only = table != nullptr;
  F.lz4 = device_stage2;  // (of either kind)
  // device-resident inputs decide the kernel variant by their address; host inputs are staged into d_in (checked where it is filled)
  F.points_misaligned = points_loc == CLDN_HIP_DEVICE ? (uint8_t)((uintptr_t)points & 3u) : (uint8_t)0;
  for (uint32_t a = 0; a < (uint32_t)kMaxAdaptive; ++a) F.mode_hint[a] = c->hint_valid ? c->hint_cache[a] : (uint8_t)0xF;
  const bool per_cloud = c->forced_clouds != 0u;  // (then forced_clouds == n_clouds)
  F.modes_forced = (!c->forced_modes.empty() || per_cloud) && n_adaptive && n_clouds;
  for (uint32_t a = 0; a < plan.n_adaptive && F.modes_forced; ++a) {
    uint8_t hint = per_cloud ? (uint8_t)0 : (uint8_t)(1u << c->forced_modes[a]);
    for (uint32_t k = 0; per_cloud && k < n_clouds; ++k) hint |= (uint8_t)(1u << c->forced_cloud_modes[(size_t)k * n_adaptive + a]);
    F.mode_hint[a] = hint;
  }
  // device-resident outputs: the probe workgroups of the piece kernel write the caller's modes array as well (a byte store
  // fits any address); where another kernel decides the modes, or the caller forced them, the copy behind the call stays
  uint8_t* const caller_modes = (out_loc == CLDN_HIP_DEVICE && !device_stage2 && !table && !F.modes_forced) ? modes : nullptr;
  F.caller_modes = caller_modes != nullptr;
  F.zero_block_reused = true;  // (known once the block is sized, see below)
  F.out_capacity = device_stage2 ? need_s1 : out_capacity;
  F.wide_adaptive = n_adaptive;
  F.wide_gorilla = wide ? c->wide_desc.n_gorilla : 0u;
  EncodeRoute R = encode_route(plan, F);

  int rc = upload_batch_shape(c, cloud_points, n_clouds, n_chunks, R.piece_pts, R.piece_pts != 0u && table != nullptr);
  if (rc != CLDN_HIP_OK) return rc;
  if (n_points && !points && !cloud_ptrs) return fail(CLDN_HIP_ERR_ARG, "points is NULL");
  if (cloud_ptrs)
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (cloud_points[k] && !cloud_ptrs[k]) return fail(CLDN_HIP_ERR_ARG, "cloud %u: NULL buffer", k);

  if (out_capacity < need)
    return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for worst-case compressed size (%llu < %llu)",
                (unsigned long long)out_capacity, (unsigned long long)need);
  if (need && !out && !deferred && !table) return fail(CLDN_HIP_ERR_ARG, "out is NULL");
  c->pending_total = 0;

  const uint32_t segs_per_chunk = R.segs_per_chunk;
  const uint64_t slot_stride = R.slot_stride;

  // one zero-filled block per call (one memset launch instead of three; none where the piece kernel clears it, see below)
  const size_t z_anchor = 256;
  const size_t z_anchor2 = z_anchor + (((size_t)(n_chunks / 1024u + 1u) * 8u + 63u) & ~size_t(63));  // framing of the LZ4 blocks
  const size_t z_flags = z_anchor2 + (((size_t)(n_chunks / 1024u + 1u) * 8u + 63u) & ~size_t(63));
  const size_t z_segs = (z_flags + (size_t)n_chunks * std::max(1u, n_adaptive) + 63u) & ~size_t(63);
  const size_t z_bytes = z_segs + std::max<size_t>(16, (size_t)n_chunks * segs_per_chunk * sizeof(Seg));
  const size_t status_cap_before = c->d_status.cap;
  if ((rc = c->d_status.ensure(z_bytes)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_offsets.ensure((size_t)(n_clouds + 1) * sizeof(uint64_t))) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_modes.ensure(std::max<size_t>(1, (size_t)n_clouds * std::max(1u, n_adaptive)))) != CLDN_HIP_OK)
    return rc;
  // Framed calls whose first launch is the piece kernel: that launch zeroes what the call needs zeroed of the block (FusedArgs::clear)
  // -- the memset was a launch and a dependent boundary on the stream in front of every call. The route says which calls those
  // are; the one that got a new allocation (known only here: the block's size follows from the route) keeps the memset too.
  R.kernel_clears = R.kernel_clears && c->d_status.cap == status_cap_before;
  if (!R.kernel_clears) HIP_TRY(hipMemsetAsync(c->d_status.p, 0, z_bytes, c->stream));
  // a batch without a single point launches no probe: its clouds commit mode 0 (DeltaVarint), like an encode() call of
  // the reference that never reaches the analysis (src/v5_codec.cpp:934-949)
  if (n_chunks == 0 && n_clouds && n_adaptive) HIP_TRY(hipMemsetAsync(c->d_modes.p, 0, (size_t)n_clouds * n_adaptive, c->stream));

  const uint8_t* d_points = (const uint8_t*)points;
  uint8_t* d_outp = (uint8_t*)out;
  if (n_chunks) {
    if ((rc = c->d_payload.ensure((size_t)n_chunks * sizeof(uint32_t))) != CLDN_HIP_OK) return rc;
    if ((rc = c->d_dst.ensure((size_t)n_chunks * sizeof(uint64_t))) != CLDN_HIP_OK) return rc;
    if ((rc = c->d_slots.ensure(std::max<size_t>(16, (size_t)n_chunks * slot_stride))) != CLDN_HIP_OK) return rc;
    {  // look-back records of k_finish: tagged with the call's epoch, so only a fresh allocation is cleared
      const void* before = c->d_finrec.p;
      if ((rc = c->d_finrec.ensure((size_t)n_chunks * 16u + (size_t)n_chunks * 32u * 8u)) != CLDN_HIP_OK) return rc;  // rec, rec2, 32 workgroup records per chunk
      if (c->d_finrec.p != before) {
        HIP_TRY(hipMemsetAsync(c->d_finrec.p, 0, c->d_finrec.cap, c->stream));
        c->finish_epoch = 0;
      }
      if (++c->finish_epoch == 0u) {  // wrapped: old records could carry the new tags
        HIP_TRY(hipMemsetAsync(c->d_finrec.p, 0, c->d_finrec.cap, c->stream));
        c->finish_epoch = 1u;
      }
    }
    for (uint32_t a = 0; a < plan.n_adaptive; ++a) {  // (WIDE: plan.n_adaptive == 0, the columns live in the chunk scratch)
      if ((rc = c->d_cols[a].ensure((size_t)n_points * plan.adaptive[a].bpv + 64)) != CLDN_HIP_OK) return rc;
      if ((rc = c->d_ranks[a].ensure((size_t)n_points * 2 + 64)) != CLDN_HIP_OK) return rc;
    }
    if (wide) {
      if ((rc = c->d_wide_scratch.ensure((size_t)n_chunks * stage1_wide_scratch_bytes())) != CLDN_HIP_OK) return rc;
      const uint32_t ng = c->plan.n_gorilla_all;
      if (ng) {
        std::vector<void*> ptrs(ng);
        for (uint32_t g = 0; g < ng; ++g) {
          if ((rc = c->d_wide_pre[g].ensure((size_t)n_points * 16 + 64)) != CLDN_HIP_OK) return rc;
          ptrs[g] = c->d_wide_pre[g].p;
        }
        if ((rc = c->d_pre_ptrs.ensure(ptrs.size() * sizeof(void*))) != CLDN_HIP_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_pre_ptrs.p, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // `ptrs` lives on this stack frame
      }
    }
    if (plan.n_gorilla) {
      void* ptrs[kMaxGorilla] = {};
      for (uint32_t g = 0; g < plan.n_gorilla; ++g) {
        // 16-byte tokens per point (generic kernel) or one window word per piece (piece kernel, kGorWinStride per chunk)
        if ((rc = c->d_pre[g].ensure(std::max((size_t)n_points * 16, (size_t)n_chunks * 256) + 64)) != CLDN_HIP_OK) return rc;
        ptrs[g] = c->d_pre[g].p;
      }
      if ((rc = c->d_pre_ptrs.ensure(sizeof(ptrs))) != CLDN_HIP_OK) return rc;
      HIP_TRY(hipMemcpyAsync(c->d_pre_ptrs.p, ptrs, sizeof(ptrs), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // `ptrs` lives on this stack frame
    }
    if (points_loc == CLDN_HIP_HOST) {
      // (gather: every cloud straight from its own buffer to its place in the batch)
      if ((rc = stage_host_input(c, points, cloud_ptrs, cloud_points, n_clouds, step, n_points * step)) != CLDN_HIP_OK) return rc;
      d_points = (const uint8_t*)c->d_in.p;
      if ((uintptr_t)d_points & 3u) return fail(CLDN_HIP_ERR_DEVICE, "staging buffer is not 4-byte aligned");  // the route assumed it is
    }
    if (out_loc == CLDN_HIP_HOST && !table) {
      if ((rc = c->d_out.ensure((size_t)need)) != CLDN_HIP_OK) return rc;
      d_outp = (uint8_t*)c->d_out.p;
    }
    if (device_stage2) {
      if ((rc = c->d_s1.ensure((size_t)need_s1)) != CLDN_HIP_OK) return rc;
      if ((rc = c->d_s1_offsets.ensure((size_t)(n_clouds + 1) * sizeof(uint64_t))) != CLDN_HIP_OK) return rc;
      if ((rc = c->d_payload2.ensure((size_t)n_chunks * sizeof(uint32_t))) != CLDN_HIP_OK) return rc;
      if ((rc = c->d_dst2.ensure((size_t)n_chunks * sizeof(uint64_t))) != CLDN_HIP_OK) return rc;
    }
  }
  EncodeLaunch L;
  memset(&L, 0, sizeof(L));
  L.plan = &plan;
  L.route = &R;
  L.stream = c->stream;
  L.points = d_points;
  L.points_end = d_points + (size_t)n_points * step;
  L.chunks = (const ChunkDesc*)c->d_chunks.p;
  L.n_chunks = n_chunks;
  L.n_clouds = n_clouds;
  L.cloud_first_chunk = (const uint32_t*)c->d_cloud_first.p;
  L.slots = (uint8_t*)c->d_slots.p;
  L.segs = (Seg*)((uint8_t*)c->d_status.p + z_segs);
  for (uint32_t a = 0; a < plan.n_adaptive; ++a) {
    L.cols.p[a] = (uint8_t*)c->d_cols[a].p;
    L.ranks[a] = (uint16_t*)c->d_ranks[a].p;
  }
  if (wide) {
    L.wide = &c->wide_desc;
    L.wide_ops_host = c->plan.ops_all.data();
    L.wide_scratch = (uint8_t*)c->d_wide_scratch.p;
    L.wide_pre = (const uint4* const*)c->d_pre_ptrs.p;
  }
  for (uint32_t g = 0; g < plan.n_gorilla; ++g) L.pre.p[g] = (const uint4*)c->d_pre[g].p;
  L.pre_out = (uint4* const*)c->d_pre_ptrs.p;
  L.chunk_payload = (uint32_t*)c->d_payload.p;
  L.chunk_dst = (uint64_t*)c->d_dst.p;
  L.stream_offsets = device_stage2 ? (uint64_t*)c->d_s1_offsets.p : (uint64_t*)c->d_offsets.p;
  // device-resident outputs: the kernels write the caller's stream_offsets / chunk_sizes arrays themselves (no copy behind
  // the call: a device-to-device copy of a few bytes costs a launch, 3-5 us of a 50 us call)
  const bool direct_offsets = out_loc == CLDN_HIP_DEVICE && !device_stage2 && !table && stream_offsets != nullptr && ((uintptr_t)stream_offsets & 7u) == 0u;
  const bool direct_sizes = out_loc == CLDN_HIP_DEVICE && !device_stage2 && !table && chunk_sizes != nullptr && ((uintptr_t)chunk_sizes & 3u) == 0u;
  if (direct_offsets) L.stream_offsets = stream_offsets;
  if (direct_sizes) L.chunk_payload = chunk_sizes;
  L.modes = (uint8_t*)c->d_modes.p;
  if (F.modes_forced) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // the previous call's upload from h_modes has to be over
    if ((rc = c->h_modes.ensure((size_t)n_clouds * n_adaptive)) != CLDN_HIP_OK) return rc;
    if (per_cloud) memcpy(c->h_modes.p, c->forced_cloud_modes.data(), (size_t)n_clouds * n_adaptive);
    for (uint32_t k = 0; !per_cloud && k < n_clouds; ++k)
      memcpy((uint8_t*)c->h_modes.p + (size_t)k * n_adaptive, c->forced_modes.data(), n_adaptive);
    HIP_TRY(hipMemcpyAsync(c->d_modes.p, c->h_modes.p, (size_t)n_clouds * n_adaptive, hipMemcpyHostToDevice,
                           c->stream));
  }
  L.fallback_flags = (uint8_t*)c->d_status.p + z_flags;
  L.caller_modes = caller_modes;
  L.fin_rec = (unsigned long long*)c->d_finrec.p;
  L.fin_rec2 = L.fin_rec + n_chunks;
  L.fin_anchor = (unsigned long long*)((uint8_t*)c->d_status.p + z_anchor);
  L.fin_epoch = c->finish_epoch;
  L.fin_ticket = (uint32_t*)c->d_status.p + 40;
  L.use_ticket = c->force_ticket ? 1u : 0u;
  L.test_timeout = c->test_timeout_once ? 1u : 0u;  // test hook (cldn_hip_debug_finish_timeout_once): this attempt reports a timeout
  c->test_timeout_once = false;
  L.contiguous_flag = (uint32_t*)c->d_status.p + 42;
  if (R.regular == ER_PIECES) {
    L.pieces = (const PieceDesc*)c->d_pieces.p;
    L.n_pieces = c->n_pieces;
    L.wgrec = L.fin_rec2 + n_chunks;
  }
  L.out = device_stage2 ? (uint8_t*)c->d_s1.p : d_outp;
  L.out_capacity = device_stage2 ? need_s1 : out_capacity;
  L.status = (uint32_t*)c->d_status.p;
  const size_t n_slots = c->slot_valid.size();
  const size_t slot = n_slots ? (size_t)(c->call_index % n_slots) : 0;
  L.events = n_slots ? &c->events[slot * 5] : nullptr;
  const bool modes_in_place = R.writes_caller_modes;  // the kernels write the caller's modes array
  rc = stage1_launch_encode(L);
  if (rc != CLDN_HIP_OK) return rc;
  // stage 2 on the device writes the call's output and its own chunk sizes
  const void* d_sizes = c->d_payload.p;  // what chunk_sizes reports
  if (device_stage2 && (rc = launch_device_stage2(c, n_chunks, n_clouds, need_s1, d_outp, out_capacity, &d_sizes)) != CLDN_HIP_OK) return rc;
  // remember this call's modes for the next call's launch hint (no synchronisation: the copy is only looked at
  // once its event has fired)
  // (a hint that is in place is refreshed with every 16th call only: it decides the launch shape, never a byte)
  if (!wide && n_adaptive && n_clouds && (size_t)n_clouds * n_adaptive <= 65536u && c->last_modes_count == 0 &&
      (!c->hint_valid || (c->call_index & 15u) == 0u)) {
    if (!c->ev_last_modes) HIP_TRY(hipEventCreateWithFlags(&c->ev_last_modes, hipEventDisableTiming));
    if (c->h_last_modes.ensure((size_t)n_clouds * n_adaptive) == CLDN_HIP_OK) {  // no copy in flight: buffer is free
      HIP_TRY(hipMemcpyAsync(c->h_last_modes.p, c->d_modes.p, (size_t)n_clouds * n_adaptive, hipMemcpyDeviceToHost,
                             c->stream));
      HIP_TRY(hipEventRecord(c->ev_last_modes, c->stream));
      c->last_modes_count = (size_t)n_clouds * n_adaptive;
      c->last_modes_fields = n_adaptive;
    }
  }
  if (n_slots) c->slot_valid[slot] = 1;
  ++c->call_index;
  if (table) {
    table->payload_base = (const uint8_t*)c->d_slots.p;
    table->chunk_stride = slot_stride;
    table->segments = (const cldn_hip_segment_t*)L.segs;
    table->segments_per_chunk = segs_per_chunk;
    table->chunk_sizes = (const uint32_t*)c->d_payload.p;
    table->not_contiguous = (const uint32_t*)c->d_status.p + 42;
    table->n_chunks = n_chunks;
    c->ct_valid = true;
    c->ct_n_chunks = n_chunks;
    c->ct_n_clouds = n_clouds;
    c->ct_slot_stride = slot_stride;
    c->ct_segs_per_chunk = segs_per_chunk;
    c->ct_segs_off = z_segs;
    c->ct_anchor_off = z_anchor;
    c->ct_need = need;
    c->enc.points = d_points;
    c->enc.cloud_points.assign(cloud_points, cloud_points + n_clouds);
    c->enc.kind = CLDN_HIP_STAGE2_NONE;
    c->enc.await_frame = true;
    if (modes && (size_t)n_clouds * n_adaptive)
      HIP_TRY(hipMemcpyAsync(modes, c->d_modes.p, (size_t)n_clouds * n_adaptive, hipMemcpyDeviceToDevice, c->stream));
    return CLDN_HIP_OK;
  }

  const size_t modes_bytes = (size_t)n_clouds * n_adaptive;
  // cldn_hip_audit_last_encode: where this call's points and streams lie
  c->enc.points = d_points;
  c->enc.streams = d_outp;
  c->enc.cloud_points.assign(cloud_points, cloud_points + n_clouds);
  c->enc.kind = zstd ? CLDN_HIP_STAGE2_ZSTD : device_stage2 ? CLDN_HIP_STAGE2_LZ4 : CLDN_HIP_STAGE2_NONE;
  c->enc.d_offsets = direct_offsets ? stream_offsets : (const uint64_t*)c->d_offsets.p;
  c->enc.offsets.clear();
  // (no device decoder reads the ZSTD frames: the audit of such a call decodes the stage-1 streams they were made from)
  c->enc.s1_streams = device_stage2 ? (const uint8_t*)c->d_s1.p : nullptr;  // (LZ4 too: cldn_hip_stream_crc32_last_encode)
  c->enc.d_s1_offsets = device_stage2 ? (const uint64_t*)c->d_s1_offsets.p : nullptr;
  if (out_loc == CLDN_HIP_DEVICE) {
    c->enc.valid = true;
    if (stream_offsets && !direct_offsets)
      HIP_TRY(hipMemcpyAsync(stream_offsets, c->d_offsets.p, (size_t)(n_clouds + 1) * sizeof(uint64_t),
                             hipMemcpyDeviceToDevice, c->stream));
    if (chunk_sizes && n_chunks && !direct_sizes)
      HIP_TRY(hipMemcpyAsync(chunk_sizes, d_sizes, (size_t)n_chunks * sizeof(uint32_t),
                             hipMemcpyDeviceToDevice, c->stream));
    if (modes && modes_bytes && !modes_in_place)
      HIP_TRY(hipMemcpyAsync(modes, c->d_modes.p, modes_bytes, hipMemcpyDeviceToDevice, c->stream));
    return CLDN_HIP_OK;
  }

  // host outputs: read the sizes back first, then exactly the produced bytes
  if ((rc = c->h_result.ensure((size_t)(n_clouds + 1) * sizeof(uint64_t) + 64)) != CLDN_HIP_OK) return rc;
  uint64_t* h_off = (uint64_t*)c->h_result.p;
  uint32_t* h_status = (uint32_t*)((uint8_t*)c->h_result.p + (size_t)(n_clouds + 1) * sizeof(uint64_t));
  HIP_TRY(hipMemcpyAsync(h_off, c->d_offsets.p, (size_t)(n_clouds + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(h_status, c->d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (*h_status & ST_FINISH_TIMEOUT) {
    // k_finish takes its workgroups in index order and waits for the records of those in front; a device that hands them
    // out in another order (or pre-empts them) makes the wait run into its bound. The ticket counter does not depend on
    // the order: the call is redone with it once, and the codec keeps it from then on.
    if (!c->force_ticket) {
      c->force_ticket = true;
      ++c->finish_retries;
      // the redone call takes this attempt's place in the timing slots (cldn_hip_codec_kernel_ms)
      --c->call_index;
      if (n_slots) c->slot_valid[slot] = 0;
      HIP_TRY(hipMemsetAsync(c->d_status.p, 0, sizeof(uint32_t), c->stream));
      return kRetryWithTicket;
    }
    return fail(CLDN_HIP_ERR_DEVICE, "k_finish: a workgroup waited too long for the sizes of the chunks before it (status 0x%x)", *h_status);
  }
  if (*h_status & ST_PALETTE_FULL) return fail(CLDN_HIP_ERR_UNSUPPORTED, kPaletteFullMessage);
  if (*h_status & ST_OUT_OVERFLOW)
    return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for uncompressed chunk");  // chunk_writer.cpp:34-36
  const uint64_t total = h_off[n_clouds];
  if (deferred) c->pending_total = total;
  else if (total) HIP_TRY(hipMemcpyAsync(out, d_outp, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if (chunk_sizes && n_chunks)
    HIP_TRY(hipMemcpyAsync(chunk_sizes, d_sizes, (size_t)n_chunks * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
  if (modes && modes_bytes) HIP_TRY(hipMemcpyAsync(modes, c->d_modes.p, modes_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (stream_offsets) memcpy(stream_offsets, h_off, (size_t)(n_clouds + 1) * sizeof(uint64_t));
  c->enc.offsets.assign(h_off, h_off + n_clouds + 1);
  c->enc.valid = true;
  return CLDN_HIP_OK;
}

static int encode_stage1_impl(cldn_hip_codec_t* c, const void* points, int points_loc, const void* const* cloud_ptrs,
                              const uint64_t* cloud_points, uint32_t n_clouds, void* out, uint64_t out_capacity, int out_loc,
                              uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes,
                              cldn_hip_chunk_table_t* table = nullptr) {
  int rc = encode_stage1_once(c, points, points_loc, cloud_ptrs, cloud_points, n_clouds, out, out_capacity, out_loc, stream_offsets,
                              chunk_sizes, modes, table);
  if (rc == kRetryWithTicket)
    rc = encode_stage1_once(c, points, points_loc, cloud_ptrs, cloud_points, n_clouds, out, out_capacity, out_loc, stream_offsets,
                            chunk_sizes, modes, table);
  return rc;
}

extern "C" {

uint32_t cldn_hip_codec_finish_retries(const cldn_hip_codec_t* c) { return c ? c->finish_retries : 0u; }

int cldn_hip_encode_stage1(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points,
                           uint32_t n_clouds, void* out, uint64_t out_capacity, int out_loc,
                           uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes) {
  return encode_stage1_impl(c, points, points_loc, nullptr, cloud_points, n_clouds, out, out_capacity, out_loc,
                            stream_offsets, chunk_sizes, modes);
}

int cldn_hip_encode_stage1_gather(cldn_hip_codec_t* c, const void* const* cloud_ptrs, const uint64_t* cloud_points,
                                  uint32_t n_clouds, void* out, uint64_t out_capacity, int out_loc,
                                  uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes) {
  if (n_clouds && !cloud_ptrs) return fail(CLDN_HIP_ERR_ARG, "cloud_ptrs is NULL");
  return encode_stage1_impl(c, nullptr, CLDN_HIP_HOST, cloud_ptrs, cloud_points, n_clouds, out, out_capacity, out_loc,
                            stream_offsets, chunk_sizes, modes);
}

int cldn_hip_encode_stage1_chunks(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points,
                                  uint32_t n_clouds, cldn_hip_chunk_table_t* table, uint8_t* modes_device) {
  if (!table) return fail(CLDN_HIP_ERR_ARG, "table is NULL");
  return encode_stage1_impl(c, points, points_loc, nullptr, cloud_points, n_clouds, nullptr, 0, CLDN_HIP_DEVICE, nullptr, nullptr,
                            modes_device, table);
}

int cldn_hip_frame_chunks(cldn_hip_codec_t* c, void* out, uint64_t out_capacity, int out_loc, uint64_t* stream_offsets,
                          uint32_t* chunk_sizes) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->ct_valid) return fail(CLDN_HIP_ERR_ARG, "frame_chunks: no chunk table (cldn_hip_encode_stage1_chunks must be this codec's last encode call)");
  if (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (out_capacity < c->ct_need)
    return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for worst-case compressed size (%llu < %llu)",
                (unsigned long long)out_capacity, (unsigned long long)c->ct_need);
  if (c->ct_need && !out) return fail(CLDN_HIP_ERR_ARG, "out is NULL");
  ENTER_DEVICE(c->device);
  int rc;
  const bool framed_encode = c->enc.await_frame;  // the table is this codec's last encode call: framing completes it for the audit
  c->enc.valid = false;
  const uint32_t n_chunks = c->ct_n_chunks, n_clouds = c->ct_n_clouds;
  uint8_t* d_outp = (uint8_t*)out;
  if (out_loc == CLDN_HIP_HOST) {
    c->pending_total = 0;
    if ((rc = c->d_out.ensure((size_t)std::max<uint64_t>(1, c->ct_need))) != CLDN_HIP_OK) return rc;
    d_outp = (uint8_t*)c->d_out.p;
  }
  if (++c->finish_epoch == 0u) {
    HIP_TRY(hipMemsetAsync(c->d_finrec.p, 0, c->d_finrec.cap, c->stream));
    c->finish_epoch = 1u;
  }
  // (anchors: zero since the encode call, or holding the values an earlier framing of the same table left -- the same ones)
  FrameLaunch F;
  F.stream = c->stream;
  F.chunks = (const ChunkDesc*)c->d_chunks.p;
  F.n_chunks = n_chunks;
  F.cloud_first_chunk = (const uint32_t*)c->d_cloud_first.p;
  F.n_clouds = n_clouds;
  F.slots = (const uint8_t*)c->d_slots.p;
  F.slot_stride = c->ct_slot_stride;
  F.segs = (const Seg*)((uint8_t*)c->d_status.p + c->ct_segs_off);
  F.segs_per_chunk = c->ct_segs_per_chunk;
  F.rec = (unsigned long long*)c->d_finrec.p;
  F.anchor = (unsigned long long*)((uint8_t*)c->d_status.p + c->ct_anchor_off);
  F.epoch = c->finish_epoch;
  F.ticket = (uint32_t*)c->d_status.p + 40;
  F.chunk_payload = (uint32_t*)c->d_payload.p;
  F.chunk_dst = (uint64_t*)c->d_dst.p;
  F.stream_offsets = (uint64_t*)c->d_offsets.p;
  F.out = d_outp;
  F.out_capacity = out_capacity;
  F.status = (uint32_t*)c->d_status.p;
  if ((rc = stage1_launch_frame(F)) != CLDN_HIP_OK) return rc;
  c->enc.streams = d_outp;
  c->enc.d_offsets = (const uint64_t*)c->d_offsets.p;
  c->enc.offsets.clear();
  if (out_loc == CLDN_HIP_DEVICE) {
    c->enc.valid = framed_encode;
    if (stream_offsets)
      HIP_TRY(hipMemcpyAsync(stream_offsets, c->d_offsets.p, (size_t)(n_clouds + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    if (chunk_sizes && n_chunks)
      HIP_TRY(hipMemcpyAsync(chunk_sizes, c->d_payload.p, (size_t)n_chunks * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return CLDN_HIP_OK;
  }
  if ((rc = c->h_result.ensure((size_t)(n_clouds + 1) * sizeof(uint64_t) + 64)) != CLDN_HIP_OK) return rc;
  uint64_t* h_off = (uint64_t*)c->h_result.p;
  uint32_t* h_status = (uint32_t*)((uint8_t*)c->h_result.p + (size_t)(n_clouds + 1) * sizeof(uint64_t));
  HIP_TRY(hipMemcpyAsync(h_off, c->d_offsets.p, (size_t)(n_clouds + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_status, c->d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (*h_status & ST_FINISH_TIMEOUT) return fail(CLDN_HIP_ERR_DEVICE, "k_finish: a workgroup waited too long (status 0x%x)", *h_status);
  if (*h_status & ST_PALETTE_FULL) return fail(CLDN_HIP_ERR_UNSUPPORTED, kPaletteFullMessage);
  if (*h_status & ST_OUT_OVERFLOW) return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for uncompressed chunk");
  const uint64_t total = h_off[n_clouds];
  if (total) HIP_TRY(hipMemcpyAsync(out, d_outp, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if (chunk_sizes && n_chunks)
    HIP_TRY(hipMemcpyAsync(chunk_sizes, c->d_payload.p, (size_t)n_chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (stream_offsets) memcpy(stream_offsets, h_off, (size_t)(n_clouds + 1) * sizeof(uint64_t));
  c->enc.offsets.assign(h_off, h_off + n_clouds + 1);
  c->enc.valid = framed_encode;
  return CLDN_HIP_OK;
}

}  // extern "C"

// The argument checks the three viz entry points share (texts of cldn_hip_viz_preprocess).
static int viz_check_args(int points_loc, int out_loc, uint32_t point_step, uint32_t xyz_offset, float resolution) {
  if ((points_loc != CLDN_HIP_HOST && points_loc != CLDN_HIP_DEVICE) ||
      (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (point_step == 0 || (uint64_t)xyz_offset + 12u > point_step)
    return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: the x/y/z triple does not fit the point (offset %u, step %u)", xyz_offset,
                point_step);
  if (!(resolution > 0.0f) || !std::isfinite(resolution))
    return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: resolution must be positive and finite");
  return CLDN_HIP_OK;
}

// points of the batch, after the per-cloud and per-batch limits (nothing is allocated or read before them)
static int viz_batch_points(const uint64_t* cloud_points, uint32_t n_clouds, uint64_t* total_out) {
  uint64_t total = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    if (cloud_points[k] >= 0xffffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "viz_preprocess: more than 2^32 - 2 points");
    total += cloud_points[k];
    if (total >= 0xffffffffull)  // (block offsets and ranks are 32-bit)
      return fail(CLDN_HIP_ERR_UNSUPPORTED, "viz_preprocess: more than 2^32 - 2 points in one batch");
  }
  // a cloud's table has viz_table_capacity(n) slots and a slot index is kept in 32 bits, 0xffffffff meaning "dropped": 2^31
  // slots (n <= 2^30) is the largest table in which every slot has an index of its own
  for (uint32_t k = 0; k < n_clouds; ++k)
    if (cloud_points[k] > (1ull << 30))
      return fail(CLDN_HIP_ERR_UNSUPPORTED, "viz_preprocess: more than 2^30 points in one cloud");
  *total_out = total;
  return CLDN_HIP_OK;
}

// The filter of a batch whose points are on the device (at least one point): cloud / block / group tables from the batch
// shape, workspace, the launches, the survivor counts back (kept_points: HOST [n_clouds]). One synchronisation.
static int viz_filter_batch(cldn_hip_codec* c, const uint8_t* d_points, const uint64_t* cloud_points, uint32_t n_clouds,
                            uint32_t point_step, uint32_t xyz_offset, float resolution, uint8_t* d_out, uint64_t* kept_points,
                            uint64_t* kept_total) {
  int rc;
  uint64_t n_points = 0, n_blocks64 = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    n_points += cloud_points[k];
    n_blocks64 += (cloud_points[k] + kVizBlockPoints - 1u) / kVizBlockPoints;
  }
  const uint32_t n_blocks = (uint32_t)n_blocks64;  // (< 2^32 points in the batch)
  const size_t kept_b = (size_t)(n_clouds + 1u) * sizeof(uint64_t);
  VizCloud* hc;
  VizBlock* hb;
  uint64_t* h_kept;
  size_t tables_b;  // what the device gets: the clouds and the blocks
  // (the previous viz call ended with a synchronisation behind its upload and its readback: the staging buffer is free)
  if ((rc = c->h_viz.ensure(carve_viz_tables(nullptr, n_clouds, n_blocks, &hc, &hb, &tables_b, &h_kept))) != CLDN_HIP_OK) return rc;
  carve_viz_tables(c->h_viz.p, n_clouds, n_blocks, &hc, &hb, &tables_b, &h_kept);
  const uint64_t limit = c->viz_group_slots ? c->viz_group_slots : (uint64_t)CLDN_HIP_VIZ_GROUP_SLOTS;
  std::vector<VizGroup> groups(1, VizGroup{0u, 0u, 0ull});
  uint64_t first = 0, max_slots = 0;
  uint32_t bi = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    const uint64_t n = cloud_points[k];
    const uint64_t cap = n ? viz_table_capacity(n) : 0u;  // zero-point clouds own no table and no block
    if (groups.back().table_slots && groups.back().table_slots + cap > limit) groups.push_back(VizGroup{bi, 0u, 0ull});
    VizGroup& G = groups.back();
    hc[k].first_point = first;
    hc[k].n_points = n;
    hc[k].tab_base = G.table_slots;
    hc[k].cap_mask = cap ? cap - 1u : 0u;
    hc[k].first_block = bi;
    hc[k].reserved = 0u;
    for (uint64_t p = 0; p < n; p += kVizBlockPoints) {
      hb[bi].cloud = k;
      hb[bi].first = (uint32_t)p;
      ++bi;
    }
    G.table_slots += cap;
    G.n_blocks = bi - G.first_block;
    max_slots = std::max(max_slots, G.table_slots);
    first += n;
  }
  if ((rc = c->d_viz_tables.ensure(tables_b)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_viz_keys.ensure((size_t)max_slots * 16u)) != CLDN_HIP_OK) return rc;  // {key, first index, pad} per slot
  if ((rc = c->d_viz_slot.ensure((size_t)n_points * 4u)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_viz_blocks.ensure((size_t)n_blocks * 4u + 16u)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_viz_bits.ensure((size_t)n_blocks * (kVizBlockPoints / 8u) + 16u)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_viz_kept.ensure(kept_b)) != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_viz_tables.p, c->h_viz.p, tables_b, hipMemcpyHostToDevice, c->stream));
  VizLaunch L;
  L.stream = c->stream;
  L.points = d_points;
  L.n_clouds = n_clouds;
  L.n_blocks = n_blocks;
  L.point_step = point_step;
  L.xyz_offset = xyz_offset;
  L.inv_res = 1.0f / resolution;  // const float inv_res = 1.0f / xyz_res (ros_msg_utils.cpp:272)
  carve_viz_tables(c->d_viz_tables.p, n_clouds, n_blocks, &L.clouds, &L.blocks, &tables_b);
  L.groups = groups.data();
  L.n_groups = (uint32_t)groups.size();
  L.keys = (unsigned long long*)c->d_viz_keys.p;
  L.slot_of = (uint32_t*)c->d_viz_slot.p;
  L.keep_bits = (unsigned long long*)c->d_viz_bits.p;
  L.block_count = (uint32_t*)c->d_viz_blocks.p;
  L.kept = (unsigned long long*)c->d_viz_kept.p;
  L.out = d_out;
  if ((rc = viz_launch(L)) != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync(h_kept, c->d_viz_kept.p, kept_b, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(kept_points, h_kept, (size_t)n_clouds * sizeof(uint64_t));
  *kept_total = h_kept[n_clouds];
  return CLDN_HIP_OK;
}

// cldn_hip_encode_stage1_viz / _gather: the filter into d_viz_out, then the encode call of the survivors from there
static int encode_stage1_viz_impl(cldn_hip_codec_t* c, const void* points, int points_loc, const void* const* cloud_ptrs,
                                  const uint64_t* cloud_points, uint32_t n_clouds, uint32_t xyz_offset, float resolution,
                                  uint64_t* kept_points, void* out, uint64_t out_capacity, int out_loc, uint64_t* stream_offsets,
                                  uint32_t* chunk_sizes, uint8_t* modes) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (n_clouds && (!cloud_points || !kept_points)) return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: NULL argument");
  if (c->forced_clouds && c->forced_clouds != n_clouds)  // (before the filter runs: the call does nothing)
    return fail(CLDN_HIP_ERR_ARG, "modes are forced for %u clouds (cldn_hip_codec_force_modes_per_cloud), the call has %u",
                c->forced_clouds, n_clouds);
  const uint32_t step = c->plan.point_step;
  int rc;
  if ((rc = viz_check_args(points_loc, out_loc, step, xyz_offset, resolution)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = viz_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  for (uint32_t k = 0; k < n_clouds; ++k) kept_points[k] = 0;
  if (n_points && !points && !cloud_ptrs) return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: NULL buffer");
  if (cloud_ptrs)
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (cloud_points[k] && !cloud_ptrs[k]) return fail(CLDN_HIP_ERR_ARG, "cloud %u: NULL buffer", k);
  // the caller sizes the output for the input counts, whatever the filter keeps (a deferred host output has no buffer yet)
  if (!(out == nullptr && out_loc == CLDN_HIP_HOST)) {
    uint64_t need = 0;
    for (uint32_t k = 0; k < n_clouds; ++k) need += cldn_hip_stage2_bound(&c->plan, cloud_points[k], c->stage2);
    if (out_capacity < need)
      return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer too small for worst-case compressed size (%llu < %llu)",
                  (unsigned long long)out_capacity, (unsigned long long)need);
  }
  if (n_points) {
    ENTER_DEVICE(c->device);
    const uint64_t bytes = n_points * step;
    const uint8_t* d_points = (const uint8_t*)points;
    if (points_loc == CLDN_HIP_HOST) {
      if ((rc = stage_host_input(c, points, cloud_ptrs, cloud_points, n_clouds, step, bytes)) != CLDN_HIP_OK) return rc;
      d_points = (const uint8_t*)c->d_in.p;
    }
    if ((rc = c->d_viz_out.ensure((size_t)bytes)) != CLDN_HIP_OK) return rc;
    uint64_t kept_total = 0;
    if ((rc = viz_filter_batch(c, d_points, cloud_points, n_clouds, step, xyz_offset, resolution, (uint8_t*)c->d_viz_out.p,
                               kept_points, &kept_total)) != CLDN_HIP_OK)
      return rc;
  }
  // (a batch without a point never allocated d_viz_out: NULL on a fresh codec, which the encode accepts for a batch whose
  // clouds are all empty -- it asks for `points` only when there are points)
  return encode_stage1_impl(c, c->d_viz_out.p, CLDN_HIP_DEVICE, nullptr, kept_points, n_clouds, out, out_capacity, out_loc,
                            stream_offsets, chunk_sizes, modes);
}

extern "C" {

int cldn_hip_viz_preprocess(cldn_hip_codec_t* c, const void* points, int points_loc, uint64_t n_points,
                            uint32_t point_step, uint32_t xyz_offset, float resolution, void* out, uint64_t out_capacity,
                            int out_loc, uint64_t* kept_points) {
  if (!c || !kept_points) return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: NULL argument");
  return cldn_hip_viz_preprocess_batch(c, points, points_loc, &n_points, 1u, point_step, xyz_offset, resolution, out, out_capacity,
                                       out_loc, kept_points);
}

int cldn_hip_viz_preprocess_batch(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points,
                                  uint32_t n_clouds, uint32_t point_step, uint32_t xyz_offset, float resolution, void* out,
                                  uint64_t out_capacity, int out_loc, uint64_t* kept_points) {
  if (!c || (n_clouds && (!cloud_points || !kept_points))) return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: NULL argument");
  c->enc.drop();
  for (uint32_t k = 0; k < n_clouds; ++k) kept_points[k] = 0;
  int rc;
  if ((rc = viz_check_args(points_loc, out_loc, point_step, xyz_offset, resolution)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = viz_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  if (n_points == 0) return CLDN_HIP_OK;
  if (!points || !out) return fail(CLDN_HIP_ERR_ARG, "viz_preprocess: NULL buffer");
  const uint64_t bytes = n_points * point_step;
  if (out_capacity < bytes)
    return fail(CLDN_HIP_ERR_CAPACITY, "viz_preprocess: output needs room for every input point (%llu < %llu)",
                (unsigned long long)out_capacity, (unsigned long long)bytes);
  ENTER_DEVICE(c->device);
  const uint8_t* d_points = (const uint8_t*)points;
  if (points_loc == CLDN_HIP_HOST) {
    if ((rc = stage_host_input(c, points, nullptr, cloud_points, n_clouds, point_step, bytes)) != CLDN_HIP_OK) return rc;
    d_points = (const uint8_t*)c->d_in.p;
  }
  uint8_t* d_out = (uint8_t*)out;
  if (out_loc == CLDN_HIP_HOST) {
    c->pending_total = 0;  // the device output buffer is reused: a deferred encode output waiting in it is gone
    if ((rc = c->d_out.ensure((size_t)bytes)) != CLDN_HIP_OK) return rc;
    d_out = (uint8_t*)c->d_out.p;
  }
  uint64_t kept_total = 0;
  if ((rc = viz_filter_batch(c, d_points, cloud_points, n_clouds, point_step, xyz_offset, resolution, d_out, kept_points,
                             &kept_total)) != CLDN_HIP_OK)
    return rc;
  if (out_loc == CLDN_HIP_HOST && kept_total)
    HIP_TRY(hipMemcpy(out, d_out, (size_t)(kept_total * point_step), hipMemcpyDeviceToHost));
  return CLDN_HIP_OK;
}

int cldn_hip_encode_stage1_viz(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points,
                               uint32_t n_clouds, uint32_t xyz_offset, float resolution, uint64_t* kept_points, void* out,
                               uint64_t out_capacity, int out_loc, uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes) {
  return encode_stage1_viz_impl(c, points, points_loc, nullptr, cloud_points, n_clouds, xyz_offset, resolution, kept_points, out,
                                out_capacity, out_loc, stream_offsets, chunk_sizes, modes);
}

int cldn_hip_encode_stage1_viz_gather(cldn_hip_codec_t* c, const void* const* cloud_ptrs, const uint64_t* cloud_points,
                                      uint32_t n_clouds, uint32_t xyz_offset, float resolution, uint64_t* kept_points, void* out,
                                      uint64_t out_capacity, int out_loc, uint64_t* stream_offsets, uint32_t* chunk_sizes,
                                      uint8_t* modes) {
  if (n_clouds && !cloud_ptrs) return fail(CLDN_HIP_ERR_ARG, "cloud_ptrs is NULL");
  return encode_stage1_viz_impl(c, nullptr, CLDN_HIP_HOST, cloud_ptrs, cloud_points, n_clouds, xyz_offset, resolution, kept_points,
                                out, out_capacity, out_loc, stream_offsets, chunk_sizes, modes);
}

int cldn_hip_codec_set_decode_fill(cldn_hip_codec_t* c, int fill) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (fill != CLDN_HIP_FILL_KEEP && fill != CLDN_HIP_FILL_ZERO) return fail(CLDN_HIP_ERR_ARG, "unknown decode fill %d", fill);
  c->decode_fill = fill;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_set_zstd_sequences(cldn_hip_codec_t* c, int on) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->zstd_sequences = on ? 1 : 0;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_zstd_sequences(const cldn_hip_codec_t* c) { return c && c->zstd_sequences ? 1 : 0; }

int cldn_hip_codec_set_zstd_matches(cldn_hip_codec_t* c, int on) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->zstd_matches = on ? 1 : 0;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_zstd_matches(const cldn_hip_codec_t* c) { return c && c->zstd_matches ? 1 : 0; }

int cldn_hip_codec_decode_stats(cldn_hip_codec_t* c, uint32_t stats[4]) {
  if (!c || !stats) return fail(CLDN_HIP_ERR_ARG, "decode_stats: NULL argument");
  memset(stats, 0, kStatPublicCount * sizeof(uint32_t));
  if (!c->d_status.p) return CLDN_HIP_OK;
  ENTER_DEVICE(c->device);
  HIP_TRY(hipMemcpyAsync(stats, (const uint32_t*)c->d_status.p + kStatFirst, kStatPublicCount * sizeof(uint32_t), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return CLDN_HIP_OK;
}

int cldn_hip_codec_fetch_output(cldn_hip_codec_t* c, void* out, uint64_t out_capacity) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (out_capacity < c->pending_total)
    return fail(CLDN_HIP_ERR_CAPACITY, "fetch_output: %llu bytes are waiting, the buffer holds %llu",
                (unsigned long long)c->pending_total, (unsigned long long)out_capacity);
  if (c->pending_total == 0) return CLDN_HIP_OK;
  if (!out) return fail(CLDN_HIP_ERR_ARG, "out is NULL");
  ENTER_DEVICE(c->device);
  HIP_TRY(hipMemcpyAsync(out, c->d_out.p, (size_t)c->pending_total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pending_total = 0;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_pipeline(cldn_hip_codec_t* c, int mode, const void* points) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (mode < 0 || mode > 2) return fail(CLDN_HIP_ERR_ARG, "pipeline mode %d out of range", mode);
  c->pipeline = mode;
  const uint8_t* p = (const uint8_t*)points;
  EncodeFacts F = {};
  F.pipeline = (uint8_t)mode;
  F.wide = c->plan.wide;
  F.points_misaligned = (uint8_t)((uintptr_t)p & 3u);
  return encode_route(c->plan.dev, F).piece_pts ? 2 : 1;
}

int cldn_hip_codec_force_modes(cldn_hip_codec_t* c, const uint8_t* modes, uint32_t n_modes) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!modes || n_modes == 0) {
    c->forced_modes.clear();
    c->forced_cloud_modes.clear();
    c->forced_clouds = 0;
    return CLDN_HIP_OK;
  }
  if (n_modes != c->plan.n_adaptive_total())
    return fail(CLDN_HIP_ERR_ARG, "force_modes: %u modes given, the plan has %u adaptive fields", n_modes,
                c->plan.n_adaptive_total());
  for (uint32_t a = 0; a < n_modes; ++a)
    if (modes[a] > 3u) return fail(CLDN_HIP_ERR_ARG, "force_modes: invalid adaptive-int mode %u", modes[a]);
  c->forced_modes.assign(modes, modes + n_modes);
  c->forced_cloud_modes.clear();
  c->forced_clouds = 0;
  return CLDN_HIP_OK;
}

int cldn_hip_codec_force_modes_per_cloud(cldn_hip_codec_t* c, const uint8_t* modes, uint32_t n_clouds) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  const uint32_t n_adaptive = c->plan.n_adaptive_total();
  const size_t n = (size_t)n_clouds * n_adaptive;
  for (size_t i = 0; modes && i < n; ++i)
    if (modes[i] > 3u) return fail(CLDN_HIP_ERR_ARG, "force_modes_per_cloud: invalid adaptive-int mode %u", modes[i]);
  c->forced_modes.clear();
  c->forced_cloud_modes.clear();
  c->forced_clouds = 0;
  if (!modes || n_clouds == 0) return CLDN_HIP_OK;  // back to probing
  c->forced_cloud_modes.assign(modes, modes + n);
  c->forced_clouds = n_clouds;  // (a plan without adaptive fields: nothing to force, the cloud count is still checked)
  return CLDN_HIP_OK;
}

int cldn_hip_decode_stage1(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                           const uint64_t* cloud_points, uint32_t n_clouds, void* points_out, uint64_t out_capacity,
                           int out_loc) {
  return cldn_hip_decode_stage1_sized(c, streams, streams_loc, stream_offsets, cloud_points, n_clouds, nullptr, CLDN_HIP_HOST,
                                      points_out, out_capacity, out_loc);
}

// what the status word of a framed decode call means to its caller
static int decode_verdict(uint32_t st) {
  if (st & ST_LZ4_REJECT) return fail(CLDN_HIP_ERR_CORRUPT, "LZ4 decompression failed");
  if (st & ST_ZSTD_REJECT) return fail(CLDN_HIP_ERR_CORRUPT, "ZSTD decompression failed");
  if (st & ST_ZSTD_HOST) return fail(CLDN_HIP_ERR_UNSUPPORTED, "ZSTD frame carries sequences or options the device decoder does not take");
  if (st & ST_CORRUPT) return fail(CLDN_HIP_ERR_CORRUPT, "malformed stage-1 stream (truncated, bad chunk size, bad mode or trailing bytes)");
  return CLDN_HIP_OK;
}

// cldn_hip_decode_lz4_gather / _zstd_gather: what they add to the contiguous calls (all HOST memory)
struct DecodeGather {
  const void* const* body_ptrs;    // [n_clouds]: `streams` of the call is NULL, stream_offsets the prefix sums of the bodies' sizes
  const void* const* expanded;     // [n_chunks] or NULL
  const uint32_t* expanded_sizes;  // [n_chunks] or NULL
  uint32_t* verdicts;              // [n_chunks] or NULL
};

// the framed decode calls. stage2 = CLDN_HIP_STAGE2_LZ4: every chunk of `streams` is [u32 block size][LZ4 block]
// (cldn_hip_decode_lz4); CLDN_HIP_STAGE2_ZSTD: [u32 frame size][ZSTD frame] (cldn_hip_decode_zstd)
static int decode_framed(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                         const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes, int chunk_sizes_loc,
                         void* points_out, uint64_t out_capacity, int out_loc, int stage2, const struct DecodeGather* gather = nullptr);

int cldn_hip_decode_stage1_sized(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                                 const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes, int chunk_sizes_loc,
                                 void* points_out, uint64_t out_capacity, int out_loc) {
  return decode_framed(c, streams, streams_loc, stream_offsets, cloud_points, n_clouds, chunk_sizes, chunk_sizes_loc, points_out,
                       out_capacity, out_loc, CLDN_HIP_STAGE2_NONE);
}

int cldn_hip_decode_lz4(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                        const uint64_t* cloud_points, uint32_t n_clouds, void* points_out, uint64_t out_capacity, int out_loc) {
  return decode_framed(c, streams, streams_loc, stream_offsets, cloud_points, n_clouds, nullptr, CLDN_HIP_HOST, points_out,
                       out_capacity, out_loc, CLDN_HIP_STAGE2_LZ4);
}

int cldn_hip_decode_zstd(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                         const uint64_t* cloud_points, uint32_t n_clouds, void* points_out, uint64_t out_capacity, int out_loc) {
  return decode_framed(c, streams, streams_loc, stream_offsets, cloud_points, n_clouds, nullptr, CLDN_HIP_HOST, points_out,
                       out_capacity, out_loc, CLDN_HIP_STAGE2_ZSTD);
}

static int decode_framed(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                         const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes, int chunk_sizes_loc,
                         void* points_out, uint64_t out_capacity, int out_loc, int stage2, const DecodeGather* gather) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if (chunk_sizes && chunk_sizes_loc != CLDN_HIP_HOST && chunk_sizes_loc != CLDN_HIP_DEVICE)
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (n_clouds && (!cloud_points || !stream_offsets)) return fail(CLDN_HIP_ERR_ARG, "NULL offsets / cloud_points");
  if ((streams_loc != CLDN_HIP_HOST && streams_loc != CLDN_HIP_DEVICE) ||
      (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  ENTER_DEVICE(c->device);
  const DevPlan& plan = c->plan.dev;
  const uint32_t step = plan.point_step;
  if (n_clouds == 0) return CLDN_HIP_OK;

  uint64_t n_points = 0, n_chunks64 = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    if (stream_offsets[k + 1] < stream_offsets[k]) return fail(CLDN_HIP_ERR_ARG, "stream_offsets must be ascending");
    n_points += cloud_points[k];
    n_chunks64 += (cloud_points[k] + kPointsPerChunk - 1) / kPointsPerChunk;
  }
  if (n_chunks64 > 0x3fffffffull) return fail(CLDN_HIP_ERR_ARG, "batch too large");
  const uint32_t n_chunks = (uint32_t)n_chunks64;
  const uint64_t need = n_points * step;
  if (out_capacity < need) return fail(CLDN_HIP_ERR_CAPACITY, "Output buffer is too small to hold the decoded data");
  if (need && !points_out) return fail(CLDN_HIP_ERR_ARG, "points_out is NULL");
  const uint64_t stream_bytes = stream_offsets[n_clouds];
  if (stream_bytes && !streams && !gather) return fail(CLDN_HIP_ERR_ARG, "streams is NULL");

  int rc;
  if ((rc = c->d_status.ensure(kStatusBytes)) != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->d_status.p, 0, kStatusBytes, c->stream));
  // tables: [stream_offsets u64 | cloud_first_point u64 | cloud_first_chunk u32] (n_clouds + 1 entries each)
  const size_t ne = (size_t)n_clouds + 1;
  const size_t table_bytes = ne * 8 + ne * 8 + ne * 4;
  // calls of a few clouds (one cloud per call: the subscriber's shape) pass the tables as a kernel argument: no upload
  const bool inline_tables = n_clouds <= kDecInlineClouds;
  uint64_t inl_so[kDecInlineClouds + 1], inl_fp[kDecInlineClouds + 1];
  uint32_t inl_fc[kDecInlineClouds + 1];
  uint32_t slot = 0;
  uint64_t* h_so = inl_so;
  uint64_t* h_fp = inl_fp;
  uint32_t* h_fc = inl_fc;
  if (!inline_tables) {
    void* stage;
    if ((rc = dec_stage_take(c, table_bytes, &slot, &stage)) != CLDN_HIP_OK) return rc;
    h_so = (uint64_t*)stage;
    h_fp = h_so + ne;
    h_fc = (uint32_t*)(h_fp + ne);
  }
  const uint64_t base_off = stream_offsets[0];
  uint64_t fp = 0;
  uint32_t fc = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    h_so[k] = stream_offsets[k] - base_off;
    h_fp[k] = fp;
    h_fc[k] = fc;
    fp += cloud_points[k];
    fc += (uint32_t)((cloud_points[k] + kPointsPerChunk - 1) / kPointsPerChunk);
  }
  h_so[n_clouds] = stream_bytes - base_off;
  h_fp[n_clouds] = fp;
  h_fc[n_clouds] = fc;
  DecodeLaunch L;
  memset(&L, 0, sizeof(L));
  uint32_t* d_sizes = nullptr;  // (where HOST chunk_sizes go)
  if ((rc = c->d_dec_meta.ensure_carved([&](void* p) { return carve_dec_meta(p, n_clouds, n_chunks, L, &d_sizes); })) != CLDN_HIP_OK) return rc;
  const bool dec_cols = c->plan.uses_v5 && plan.n_adaptive >= 1u && plan.n_adaptive <= kSoMaxFields;
  for (uint32_t a = 0; a < 8u; ++a)
    if (dec_cols && a < plan.n_adaptive && plan.adaptive[a].bpv <= 4u &&
        (rc = c->d_dec_cols[a].ensure((size_t)n_points * plan.adaptive[a].bpv + 64)) != CLDN_HIP_OK)
      return rc;
  if (!inline_tables && (rc = dec_stage_send(c, slot, c->d_dec_meta.p, table_bytes)) != CLDN_HIP_OK) return rc;  // the three tables

  const uint8_t* d_streams = (const uint8_t*)streams + base_off;
  if (streams_loc == CLDN_HIP_HOST) {
    if ((rc = c->d_in.ensure((size_t)std::max<uint64_t>(1, stream_bytes - base_off))) != CLDN_HIP_OK) return rc;
    if (gather) {  // every body from where it lies to its place: no gathering copy on the host
      for (uint32_t k = 0; k < n_clouds; ++k)
        if (stream_offsets[k + 1] > stream_offsets[k])
          HIP_TRY(hipMemcpyAsync((uint8_t*)c->d_in.p + (stream_offsets[k] - base_off), gather->body_ptrs[k],
                                 (size_t)(stream_offsets[k + 1] - stream_offsets[k]), hipMemcpyHostToDevice, c->stream));
    } else if (stream_bytes > base_off) {
      HIP_TRY(hipMemcpyAsync(c->d_in.p, (const uint8_t*)streams + base_off, (size_t)(stream_bytes - base_off),
                             hipMemcpyHostToDevice, c->stream));
    }
    d_streams = (const uint8_t*)c->d_in.p;
  }
  uint8_t* d_outp = (uint8_t*)points_out;
  if (out_loc == CLDN_HIP_HOST) {
    c->pending_total = 0;  // the device output buffer is reused: a deferred encode output waiting in it is gone
    if ((rc = c->d_out.ensure((size_t)std::max<uint64_t>(1, need))) != CLDN_HIP_OK) return rc;
    d_outp = (uint8_t*)c->d_out.p;
    // bytes of a point that no field covers keep the caller's content (src/field_decoder.cpp:72-76): bring it along
    if (need && c->plan.has_padding) {
      if (c->decode_fill == CLDN_HIP_FILL_ZERO) HIP_TRY(hipMemsetAsync(d_outp, 0, (size_t)need, c->stream));
      else HIP_TRY(hipMemcpyAsync(d_outp, points_out, (size_t)need, hipMemcpyHostToDevice, c->stream));
    }
  }

  L.plan = &plan;
  L.stream = c->stream;
  L.uses_v5 = c->plan.uses_v5 ? 1u : 0u;
  L.streams = d_streams;
  if (inline_tables) {
    L.h_stream_offsets = h_so;
    L.h_cloud_first_point = h_fp;
    L.h_cloud_first_chunk = h_fc;
  }
  L.n_clouds = n_clouds;
  L.n_chunks = n_chunks;
  if (dec_cols && plan.n_adaptive == 1u && n_chunks) {  // slice records of k_sections_cols_fast
    const void* before = c->d_dec_rec.p;
    if ((rc = c->d_dec_rec.ensure((size_t)n_chunks * 48u * 16u)) != CLDN_HIP_OK) return rc;
    if (c->d_dec_rec.p != before || ++c->dec_epoch == 0u) {  // fresh memory, or the tags have wrapped
      HIP_TRY(hipMemsetAsync(c->d_dec_rec.p, 0, c->d_dec_rec.cap, c->stream));
      c->dec_epoch = 1u;
    }
    L.slice_rec = (unsigned long long*)c->d_dec_rec.p;
    L.slice_epoch = c->dec_epoch;
  }
  if (chunk_sizes && n_chunks) {
    if (chunk_sizes_loc == CLDN_HIP_DEVICE) {
      L.chunk_sizes = chunk_sizes;
    } else {  // (pageable source: the copy is over when the call returns)
      HIP_TRY(hipMemcpyAsync(d_sizes, chunk_sizes, (size_t)n_chunks * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      L.chunk_sizes = d_sizes;
    }
  }
  for (uint32_t a = 0; a < 8u; ++a)
    L.cols[a] = (dec_cols && a < plan.n_adaptive && plan.adaptive[a].bpv <= 4u) ? (uint8_t*)c->d_dec_cols[a].p : nullptr;
  // sections side by side (stage1_decode_sections_w.h): L.dsec, L.done_cnt, L.secs_ok; NULL without them
  if (c->plan.uses_v5 && plan.n_adaptive >= 1u && plan.n_adaptive <= kSoMaxFields && n_chunks &&
      (rc = c->d_dec_secs.ensure_carved([&](void* p) { return carve_dec_secs(p, plan.n_adaptive, n_chunks, L); })) != CLDN_HIP_OK)
    return rc;
  // LZ4 chunks: a slot per chunk with the capacity the host path gives LZ4_decompress_safe (cloudini.cpp, PointcloudDecoder::
  // decodeInto: the bound of a chunk's stage-1 payload + 60); the decoders then read the slots as their stream buffer
  uint64_t decoder_stream_bytes = stream_bytes - base_off;
  const bool lz4 = stage2 == CLDN_HIP_STAGE2_LZ4, zstd = stage2 == CLDN_HIP_STAGE2_ZSTD;
  ZstdDecodeLaunch Z;  // (the ZSTD part of this call: L.zstd points at it until stage1_launch_decode has returned)
  memset(&Z, 0, sizeof(Z));
  if ((lz4 || zstd) && n_chunks) {
    const uint64_t capacity = cldn_hip_stage1_bound(&c->plan, kPointsPerChunk) + 60u;
    if (capacity > 0x7fffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "decode_%s: a chunk of this schema may exceed 2 GiB", lz4 ? "lz4" : "zstd");
    const uint64_t stride = (capacity + 15u) & ~uint64_t(15);
    decoder_stream_bytes = stride * n_chunks;
    if ((rc = c->d_lzd_slots.ensure((size_t)decoder_stream_bytes + 256u)) != CLDN_HIP_OK) return rc;
    L.lz4_slots = (uint8_t*)c->d_lzd_slots.p;
    L.lz4_slot_stride = stride;
    L.lz4_capacity = (uint32_t)capacity;
    if (zstd) {  // the frames' block records, sized from the bytes of the call
      if (stream_bytes - base_off > 0x7fffffffull * 64u) return fail(CLDN_HIP_ERR_UNSUPPORTED, "decode_zstd: streams of more than 128 GiB");
      const bool seq_on = c->zstd_sequences != 0;  // (frames with sequences: their scratch mirrors the slots)
      const uint32_t max_recs = ZstdDecodeLaunch::records_for(n_chunks, stream_bytes - base_off, decoder_stream_bytes, seq_on);
      // [workspace | Z.sizes: u32 per chunk]
      if ((rc = c->d_zsd_ws.ensure_carved([&](void* p) { return carve_zstd_chunks(p, max_recs, n_chunks, seq_on, decoder_stream_bytes, Z); })) != CLDN_HIP_OK)
        return rc;
      Z.stream = c->stream;
      Z.frames = d_streams;
      Z.n_frames = n_chunks;
      Z.out = L.lz4_slots;
      Z.status = (uint32_t*)c->d_status.p;
      Z.chunks = L.chunks;
      Z.slot_stride = stride;
      Z.capacity = (uint32_t)capacity;
      L.zstd = &Z;
    }
    if (gather) {
      // expanded chunks: their payloads go up into their slots now (no kernel of the call writes an expanded chunk's slot),
      // their sizes into the table k_stage2_hold_expanded / _place_expanded read; the verdicts lie behind it
      uint32_t* d_exp = nullptr;
      if ((rc = c->d_s2_gather.ensure_carved([&](void* p) { return carve_s2_gather(p, n_chunks, &d_exp, &L.verdicts); })) != CLDN_HIP_OK) return rc;
      uint32_t gslot;
      void* gstage;
      if ((rc = dec_stage_take(c, (size_t)n_chunks * 4u, &gslot, &gstage)) != CLDN_HIP_OK) return rc;
      uint32_t* const h_exp = (uint32_t*)gstage;
      for (uint32_t k = 0; k < n_chunks; ++k) {
        const bool given = gather->expanded && gather->expanded[k];
        h_exp[k] = given ? gather->expanded_sizes[k] : kNotExpanded;
        if (given && h_exp[k] > capacity)
          return fail(CLDN_HIP_ERR_ARG, "expanded chunk %u has %u bytes: more than a slot's %llu", k, h_exp[k], (unsigned long long)capacity);
      }
      if ((rc = dec_stage_send(c, gslot, d_exp, (size_t)n_chunks * 4u)) != CLDN_HIP_OK) return rc;
      for (uint32_t k = 0; k < n_chunks; ++k)
        if (h_exp[k] != kNotExpanded && h_exp[k] != 0u)
          HIP_TRY(hipMemcpyAsync(L.lz4_slots + (uint64_t)k * stride, gather->expanded[k], h_exp[k], hipMemcpyHostToDevice, c->stream));
      L.expanded_sizes = d_exp;
    }
  }
  if (plan.varint_and_raw && n_chunks) {  // one bit per stream byte + a word per chunk (k_mark_token_ends)
    if ((rc = c->d_dec_bits.ensure((size_t)(decoder_stream_bytes / 8u) + (size_t)n_chunks * 4u + 256u)) != CLDN_HIP_OK) return rc;
    L.token_ends = (uint32_t*)c->d_dec_bits.p;
  }
  L.out = d_outp;
  L.fill_zero = c->decode_fill == CLDN_HIP_FILL_ZERO ? 1u : 0u;
  L.status = (uint32_t*)c->d_status.p;
  if (c->plan.wide) {  // the serial decoder with the plan in device memory; its per-op state: 16 bytes per op and chunk
    if ((rc = c->d_wide_state.ensure((size_t)std::max(1u, n_chunks) * std::max<size_t>(1, c->plan.ops_all.size()) * 16u)) != CLDN_HIP_OK) return rc;
    L.wide = &c->wide_desc;
    L.wide_state = c->d_wide_state.p;
  }
  if (c->dec_stats_chunks && c->ev_dec_stats && hipEventQuery(c->ev_dec_stats) == hipSuccess) {  // an earlier call's counters have landed
    const uint32_t* hs = (const uint32_t*)c->h_dec_stats.p;
    const bool none_serial = hs[kStatSerialChunks - kStatFirst] == 0u && hs[kStatSerialSections - kStatFirst] == 0u;
    c->dec_palette_hint = hs[kStatFoldedByGuess - kStatFirst] == c->dec_stats_chunks && none_serial;
    c->dec_dv_hint = hs[kStatDvMode - kStatFirst] == 0u ? 1u : (hs[kStatDvChunks - kStatFirst] == c->dec_stats_chunks && none_serial ? 2u : 0u);
    c->dec_stats_chunks = 0;
    c->dec_stats_seen = true;
  }
  L.palette_hint = c->dec_palette_hint ? 1u : 0u;
  L.dv_hint = c->dec_dv_hint;
  // small batches: the point kernel's pieces spread over several workgroups per chunk (SPLIT launches) want their workspace
  L.wp_parts = c->test_split_parts == 0u ? wp_split_parts(n_chunks) : c->test_split_parts;
  if (!c->plan.wide && L.wp_parts > 1u) {
    uint64_t chunk_bound = (uint64_t)kPointsPerChunk * c->plan.ref_max_point_bytes;
    if (c->plan.uses_v5) chunk_bound += (uint64_t)c->plan.fields.size() * 32u + 1024u;
    const uint64_t maxp = chunk_bound / 992u + 3u;  // (kWpPiece, stage1_decode_wave.h: pieces of 62 units)
    if (maxp <= 4096u) {
      if ((rc = c->d_dec_split.ensure(wp_split_bytes(n_chunks, (uint32_t)maxp))) != CLDN_HIP_OK) return rc;
      L.wp_split = c->d_dec_split.p;
      L.wp_maxp = (uint32_t)maxp;
    }
  }
  L.events = c->dec_events[0] ? c->dec_events : nullptr;
  if (L.events) {
    (void)hipEventRecord(L.events[0], c->stream);
    (void)hipEventRecord(L.events[1], c->stream);  // (recorded again in front of the regular-stream kernel, if the call has one)
    (void)hipEventRecord(L.events[2], c->stream);
  }
  ++c->dec_call_index;
  c->dec_trace = {n_chunks, c->d_dec_meta.p, L.reg_end, L.reg_end_pre, L.slices_done, L.sec_done, L.sec_cols};
  if ((rc = stage1_launch_decode(L)) != CLDN_HIP_OK) return rc;
  if (L.events) {
    (void)hipEventRecord(L.events[3], c->stream);
    c->dec_events_valid = true;
  }
  // (the counters of every 4th call are enough once one copy has landed: the hints pick a launch shape, never a byte)
  if (n_chunks && c->plan.uses_v5 && c->dec_stats_chunks == 0 && (!c->dec_stats_seen || (c->dec_call_index & 3u) == 0u) &&
      c->h_dec_stats.ensure(64) == CLDN_HIP_OK) {  // (no copy in flight)
    if (!c->ev_dec_stats) HIP_TRY(hipEventCreateWithFlags(&c->ev_dec_stats, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(c->h_dec_stats.p, (const uint32_t*)c->d_status.p + kStatFirst, kStatCount * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->ev_dec_stats, c->stream));
    c->dec_stats_chunks = n_chunks;
  }

  if (out_loc == CLDN_HIP_DEVICE && !gather) return CLDN_HIP_OK;
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->d_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  if (gather && gather->verdicts && L.verdicts)  // (in front of the verdict of the call: a caller that retries reads them)
    HIP_TRY(hipMemcpyAsync(gather->verdicts, L.verdicts, (size_t)n_chunks * 4u, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((rc = decode_verdict(st)) != CLDN_HIP_OK) return rc;
  if (need && out_loc == CLDN_HIP_HOST) HIP_TRY(hipMemcpy(points_out, d_outp, (size_t)need, hipMemcpyDeviceToHost));
  return CLDN_HIP_OK;
}

static int decode_gather(cldn_hip_codec_t* c, const void* const* body_ptrs, const uint64_t* body_sizes, const uint64_t* cloud_points,
                         uint32_t n_clouds, const uint32_t* chunk_sizes, const void* const* expanded, const uint32_t* expanded_sizes,
                         uint32_t* verdicts, void* points_out, uint64_t out_capacity, int out_loc, int stage2) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (n_clouds && (!body_ptrs || !body_sizes || !cloud_points)) return fail(CLDN_HIP_ERR_ARG, "NULL body_ptrs / body_sizes / cloud_points");
  if ((expanded != nullptr) != (expanded_sizes != nullptr)) return fail(CLDN_HIP_ERR_ARG, "expanded and expanded_sizes go together");
  std::vector<uint64_t> offsets((size_t)n_clouds + 1, 0);
  for (uint32_t k = 0; k < n_clouds; ++k) {
    if (body_sizes[k] && !body_ptrs[k]) return fail(CLDN_HIP_ERR_ARG, "body %u is NULL", k);
    if (__builtin_add_overflow(offsets[k], body_sizes[k], &offsets[k + 1])) return fail(CLDN_HIP_ERR_ARG, "batch too large");
  }
  const DecodeGather G = {body_ptrs, expanded, expanded_sizes, verdicts};
  return decode_framed(c, nullptr, CLDN_HIP_HOST, offsets.data(), cloud_points, n_clouds, chunk_sizes, CLDN_HIP_HOST, points_out,
                       out_capacity, out_loc, stage2, &G);
}

int cldn_hip_decode_lz4_gather(cldn_hip_codec_t* c, const void* const* body_ptrs, const uint64_t* body_sizes, const uint64_t* cloud_points,
                               uint32_t n_clouds, const uint32_t* chunk_sizes, const void* const* expanded, const uint32_t* expanded_sizes,
                               uint32_t* verdicts, void* points_out, uint64_t out_capacity, int out_loc) {
  return decode_gather(c, body_ptrs, body_sizes, cloud_points, n_clouds, chunk_sizes, expanded, expanded_sizes, verdicts, points_out,
                       out_capacity, out_loc, CLDN_HIP_STAGE2_LZ4);
}

int cldn_hip_decode_zstd_gather(cldn_hip_codec_t* c, const void* const* body_ptrs, const uint64_t* body_sizes, const uint64_t* cloud_points,
                                uint32_t n_clouds, const uint32_t* chunk_sizes, const void* const* expanded, const uint32_t* expanded_sizes,
                                uint32_t* verdicts, void* points_out, uint64_t out_capacity, int out_loc) {
  return decode_gather(c, body_ptrs, body_sizes, cloud_points, n_clouds, chunk_sizes, expanded, expanded_sizes, verdicts, points_out,
                       out_capacity, out_loc, CLDN_HIP_STAGE2_ZSTD);
}

// cldn_hip_lz4_decompress / cldn_hip_zstd_decompress: span k of `src`, an LZ4 block or a ZSTD frame, decodes into span k of `out`.
// kind = CLDN_HIP_STAGE2_LZ4 / _ZSTD decides the name in the error texts, the launch (ZSTD: with its workspace) and the verdict.
static int decompress_spans(cldn_hip_codec_t* c, int kind, const void* src, int src_loc, const uint64_t* src_offsets, uint32_t n,
                            void* out, int out_loc, const uint64_t* out_offsets, uint32_t* sizes) {
  const bool zstd = kind == CLDN_HIP_STAGE2_ZSTD;
  const char* const who = zstd ? "zstd" : "lz4";
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if ((src_loc != CLDN_HIP_HOST && src_loc != CLDN_HIP_DEVICE) || (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (n == 0) return CLDN_HIP_OK;
  if (!src_offsets || !out_offsets || !sizes) return fail(CLDN_HIP_ERR_ARG, "%s_decompress: NULL offsets / sizes", who);
  if (out_loc == CLDN_HIP_DEVICE && ((uintptr_t)sizes & 3u)) return fail(CLDN_HIP_ERR_ARG, "%s_decompress: device sizes must be 4-byte aligned", who);
  for (uint32_t k = 0; k < n; ++k) {
    if (src_offsets[k + 1] < src_offsets[k] || out_offsets[k + 1] < out_offsets[k])
      return fail(CLDN_HIP_ERR_ARG, "%s_decompress: offsets must be ascending", who);
    if (src_offsets[k + 1] - src_offsets[k] > 0x7fffffffull || out_offsets[k + 1] - out_offsets[k] > 0x7fffffffull)
      return fail(CLDN_HIP_ERR_UNSUPPORTED, "%s_decompress: block or output span of more than 2 GiB", who);
  }
  const uint64_t b0 = src_offsets[0], b_bytes = src_offsets[n] - b0;
  const uint64_t o0 = out_offsets[0], o_bytes = out_offsets[n] - o0;
  if ((b_bytes && !src) || (o_bytes && !out)) return fail(CLDN_HIP_ERR_ARG, "%s_decompress: NULL buffer", who);
  ENTER_DEVICE(c->device);
  int rc;
  if ((rc = c->d_status.ensure(kStatusBytes)) != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->d_status.p, 0, kStatusBytes, c->stream));
  // tables: [src offsets u64 | out offsets u64] relative to the first block / span, [sizes u32] for HOST outputs
  const size_t ne = (size_t)n + 1;
  SpanTables T;
  if ((rc = c->d_lzd_tables.ensure_carved([&](void* p) { return carve_span_tables(p, n, T); })) != CLDN_HIP_OK) return rc;
  // (staged through the decode calls' ring of page-locked buffers: no wait for the stream unless the ring has gone round)
  uint32_t slot;
  void* stage;
  if ((rc = dec_stage_take(c, ne * 16u, &slot, &stage)) != CLDN_HIP_OK) return rc;
  uint64_t* h_bo = (uint64_t*)stage;
  uint64_t* h_oo = h_bo + ne;
  for (size_t k = 0; k < ne; ++k) {
    h_bo[k] = src_offsets[k] - b0;
    h_oo[k] = out_offsets[k] - o0;
  }
  if ((rc = dec_stage_send(c, slot, T.src_offsets, ne * 16u)) != CLDN_HIP_OK) return rc;  // both offset tables
  const uint8_t* d_src = (const uint8_t*)src + b0;
  if (src_loc == CLDN_HIP_HOST) {
    if ((rc = c->d_in.ensure((size_t)std::max<uint64_t>(1, b_bytes))) != CLDN_HIP_OK) return rc;
    if (b_bytes) HIP_TRY(hipMemcpyAsync(c->d_in.p, (const uint8_t*)src + b0, (size_t)b_bytes, hipMemcpyHostToDevice, c->stream));
    d_src = (const uint8_t*)c->d_in.p;
  }
  uint8_t* d_outp = (uint8_t*)out + o0;
  uint32_t* d_sizes = sizes;
  if (out_loc == CLDN_HIP_HOST) {
    c->pending_total = 0;  // the device output buffer is reused: a deferred encode output waiting in it is gone
    if ((rc = c->d_out.ensure((size_t)std::max<uint64_t>(1, o_bytes))) != CLDN_HIP_OK) return rc;
    d_outp = (uint8_t*)c->d_out.p;
    // bytes of a span behind the decoded ones keep the caller's content: bring it along
    if (o_bytes) HIP_TRY(hipMemcpyAsync(d_outp, (const uint8_t*)out + o0, (size_t)o_bytes, hipMemcpyHostToDevice, c->stream));
    d_sizes = T.sizes;
  }
  if (zstd) {
    const bool seq_on = c->zstd_sequences != 0;  // (frames with sequences: their scratch mirrors the output spans)
    const uint32_t max_recs = ZstdDecodeLaunch::records_for(n, b_bytes, o_bytes, seq_on);
    if ((rc = c->d_zsd_ws.ensure(ZstdDecodeLaunch::workspace_bytes(max_recs, n, seq_on, o_bytes))) != CLDN_HIP_OK) return rc;
    ZstdDecodeLaunch L;
    memset(&L, 0, sizeof(L));
    L.carve(c->d_zsd_ws.p, max_recs, n, seq_on, o_bytes);
    L.stream = c->stream;
    L.frames = d_src;
    L.frame_offsets = T.src_offsets;
    L.n_frames = n;
    L.out = d_outp;
    L.out_offsets = T.out_offsets;
    L.sizes = d_sizes;
    L.status = (uint32_t*)c->d_status.p;
    rc = zstd_launch_decode(L);
  } else {
    Lz4DecompressLaunch L;
    L.stream = c->stream;
    L.blocks = d_src;
    L.block_offsets = T.src_offsets;
    L.n_blocks = n;
    L.out = d_outp;
    L.out_offsets = T.out_offsets;
    L.sizes = d_sizes;
    L.status = (uint32_t*)c->d_status.p;
    rc = lz4_launch_decompress(L);
  }
  if (rc != CLDN_HIP_OK || out_loc == CLDN_HIP_DEVICE) return rc;
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->d_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(sizes, d_sizes, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream));
  if (o_bytes) HIP_TRY(hipMemcpyAsync((uint8_t*)out + o0, d_outp, (size_t)o_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st & ST_CORRUPT)
    return fail(CLDN_HIP_ERR_CORRUPT, zstd ? "ZSTD decompression failed (sizes[k] == 0xffffffff marks the frames)"
                                           : "LZ4 decompression failed (sizes[k] == 0xffffffff marks the blocks)");
  if (zstd && (st & ST_ZSTD_HOST))
    return fail(CLDN_HIP_ERR_UNSUPPORTED, "ZSTD frame carries sequences or options the device decoder does not take (sizes[k] == 0xfffffffe marks the frames)");
  return CLDN_HIP_OK;
}

int cldn_hip_lz4_decompress(cldn_hip_codec_t* c, const void* blocks, int blocks_loc, const uint64_t* block_offsets, uint32_t n_blocks,
                            void* out, int out_loc, const uint64_t* out_offsets, uint32_t* sizes) {
  return decompress_spans(c, CLDN_HIP_STAGE2_LZ4, blocks, blocks_loc, block_offsets, n_blocks, out, out_loc, out_offsets, sizes);
}

int cldn_hip_zstd_decompress(cldn_hip_codec_t* c, const void* frames, int frames_loc, const uint64_t* frame_offsets, uint32_t n_frames,
                             void* out, int out_loc, const uint64_t* out_offsets, uint32_t* sizes) {
  return decompress_spans(c, CLDN_HIP_STAGE2_ZSTD, frames, frames_loc, frame_offsets, n_frames, out, out_loc, out_offsets, sizes);
}

int cldn_hip_decode_stage1_unframed(cldn_hip_codec_t* c, const void* payload, uint64_t size, int payload_loc,
                                    void* points_out, uint64_t out_capacity, int out_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if ((payload_loc != CLDN_HIP_HOST && payload_loc != CLDN_HIP_DEVICE) || (out_loc != CLDN_HIP_HOST && out_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (c->plan.uses_v5) return fail(CLDN_HIP_ERR_ARG, "unframed streams (wire version 2) never use the V5 codec");
  if (size == 0) return CLDN_HIP_OK;
  if (!payload) return fail(CLDN_HIP_ERR_ARG, "payload is NULL");
  if (size > 0xffffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "unframed payload of more than 4 GiB");
  ENTER_DEVICE(c->device);
  const uint32_t step = c->plan.dev.point_step;
  const uint64_t cap_points = std::min<uint64_t>(out_capacity / step, 0xffffffffull);
  int rc;
  if ((rc = c->d_status.ensure(kStatusBytes)) != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->d_status.p, 0, kStatusBytes, c->stream));
  if ((rc = c->d_dec_meta.ensure(256)) != CLDN_HIP_OK) return rc;
  const uint8_t* d_payload = (const uint8_t*)payload;
  if (payload_loc == CLDN_HIP_HOST) {
    if ((rc = c->d_in.ensure((size_t)size)) != CLDN_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_in.p, payload, (size_t)size, hipMemcpyHostToDevice, c->stream));
    d_payload = (const uint8_t*)c->d_in.p;
  }
  uint8_t* d_outp = (uint8_t*)points_out;
  const uint64_t out_bytes = cap_points * step;
  if (out_loc == CLDN_HIP_HOST) {
    c->pending_total = 0;
    if ((rc = c->d_out.ensure((size_t)std::max<uint64_t>(1, out_bytes))) != CLDN_HIP_OK) return rc;
    d_outp = (uint8_t*)c->d_out.p;
    // how many points the stream holds is not known beforehand: every byte the decoder does not write keeps the caller's
    // content (uncovered bytes of a point, and all points behind the last decoded one)
    if (out_bytes) HIP_TRY(hipMemcpyAsync(d_outp, points_out, (size_t)out_bytes, hipMemcpyHostToDevice, c->stream));
  }
  if (c->plan.wide && (rc = c->d_wide_state.ensure(std::max<size_t>(1, c->plan.ops_all.size()) * 16u)) != CLDN_HIP_OK) return rc;
  if ((rc = stage1_launch_decode_unframed(c->plan.dev, c->stream, d_payload, (uint32_t)size, (uint32_t)cap_points, c->d_dec_meta.p,
                                          d_outp, (uint32_t*)c->d_status.p, c->plan.wide ? &c->wide_desc : nullptr,
                                          c->d_wide_state.p)) != CLDN_HIP_OK)
    return rc;
  if (out_loc == CLDN_HIP_DEVICE) return CLDN_HIP_OK;
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->d_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st & ST_CORRUPT) return fail(CLDN_HIP_ERR_CORRUPT, "malformed stage-1 stream (truncated point, or more points than the output holds)");
  if (out_bytes) HIP_TRY(hipMemcpy(points_out, d_outp, (size_t)out_bytes, hipMemcpyDeviceToHost));
  return CLDN_HIP_OK;
}

}  // extern "C"

// ---- audit: per-field error report (audit_kernels.hip) ----

// the schema's fields as the kernel wants them; limit == NULL: a field's resolution, else 0
static int audit_fields(const cldn_hip_plan& P, const double* limit, std::vector<AuditField>* out) {
  out->resize(P.fields.size());
  for (size_t i = 0; i < P.fields.size(); ++i) {
    const cldn_hip_field_t& f = P.fields[i];
    const int sz = size_of_type(f.type);
    if (f.offset == 0xffffffffu) return fail(CLDN_HIP_ERR_ARG, "audit: field %zu is decoded but not stored (kDecodeButSkipStore)", i);
    if (sz == 0 || (uint64_t)f.offset + (uint64_t)sz > P.point_step)
      return fail(CLDN_HIP_ERR_ARG, "audit: field %zu (offset %u, %d bytes) exceeds point_step %u", i, f.offset, sz, P.point_step);
    const double lim = limit ? limit[i] : (f.has_resolution ? (double)f.resolution : 0.0);
    if (!(lim >= 0.0)) return fail(CLDN_HIP_ERR_ARG, "audit: limit of field %zu must be >= 0 and not NaN", i);
    AuditField& a = (*out)[i];
    memset(&a, 0, sizeof(a));
    a.offset = f.offset;
    a.size = (uint8_t)sz;
    a.is_float = (f.type == 7 || f.type == 8) ? 1 : 0;
    a.limit = lim;
  }
  return CLDN_HIP_OK;
}

// ---- what the three report calls share: argument checks, tables up, the report's place, host points up ----

// `anything`: the plan has something to report
static int report_check(const char* who, bool anything, uint32_t n_clouds, const void* report, int report_loc) {
  if (report_loc != CLDN_HIP_HOST && report_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (n_clouds && anything && !report) return fail(CLDN_HIP_ERR_ARG, "%s: report is NULL", who);
  if (report_loc == CLDN_HIP_DEVICE && ((uintptr_t)report & 7u)) return fail(CLDN_HIP_ERR_ARG, "%s: a device report must be 8-byte aligned", who);
  return CLDN_HIP_OK;
}

// What the host-built tables of a call are cut from
struct ReportBatch {
  const uint64_t* cloud_points;
  uint32_t n_clouds, n_fields;
};
// One section of the tables of a call: `bytes` copied from `src`, or written in place by `fill` when src is NULL. A section of
// 0 bytes is left out and its `dev` stays NULL.
struct TableSection {
  size_t bytes;
  const void* src;
  void (*fill)(const ReportBatch& B, void* h);
  const uint8_t* dev;  // out: the section in d_audit_tab
};
// the field table goes to the device only when it does not fit the kernel arguments
template <class F>
static TableSection field_section(const std::vector<F>& fields) {
  return TableSection{fields.size() > kReportArgFields ? fields.size() * sizeof(F) : 0u, fields.data(), nullptr, nullptr};
}

// Tables up: the sections back to back, each rounded up to 64 bytes, through the pinned h_audit into d_audit_tab in one copy
static int upload_tables(cldn_hip_codec* c, const ReportBatch& B, TableSection* sec, size_t n_sections) {
  if (c->ev_audit) HIP_TRY(hipEventSynchronize(c->ev_audit));  // the previous call's upload has left the staging buffer
  else HIP_TRY(hipEventCreateWithFlags(&c->ev_audit, hipEventDisableTiming));
  size_t total = 0;
  for (size_t i = 0; i < n_sections; ++i) total += (sec[i].bytes + 63u) & ~size_t(63);
  int rc;
  if ((rc = c->h_audit.ensure(total)) != CLDN_HIP_OK) return rc;
  if ((rc = c->d_audit_tab.ensure(total)) != CLDN_HIP_OK) return rc;
  size_t at = 0;
  for (size_t i = 0; i < n_sections; ++i) {
    if (sec[i].bytes == 0) continue;
    uint8_t* h = (uint8_t*)c->h_audit.p + at;
    if (sec[i].src) memcpy(h, sec[i].src, sec[i].bytes);
    else sec[i].fill(B, h);
    sec[i].dev = (const uint8_t*)c->d_audit_tab.p + at;
    at += (sec[i].bytes + 63u) & ~size_t(63);
  }
  HIP_TRY(hipMemcpyAsync(c->d_audit_tab.p, c->h_audit.p, total, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->ev_audit, c->stream));
  return CLDN_HIP_OK;
}

// The cloud table of a batch, as the three kernels read it
static void fill_clouds(const ReportBatch& B, void* h) {
  ReportCloud* hc = (ReportCloud*)h;
  uint64_t first = 0;
  for (uint32_t k = 0; k < B.n_clouds; ++k) {
    hc[k] = ReportCloud{first, B.cloud_points[k]};
    first += B.cloud_points[k];
  }
}
static TableSection cloud_section(const ReportBatch& B) {
  return TableSection{(size_t)B.n_clouds * sizeof(ReportCloud), nullptr, fill_clouds, nullptr};
}

// The audit's and the sweep's workgroups: blocks of kReportBlockPoints points, cut per cloud
static void fill_blocks(const ReportBatch& B, void* h) {
  ReportBlock* hb = (ReportBlock*)h;
  for (uint32_t k = 0; k < B.n_clouds; ++k) {
    const uint32_t nb = (uint32_t)((B.cloud_points[k] + kReportBlockPoints - 1u) / kReportBlockPoints);
    for (uint32_t j = 0; j < nb; ++j) *hb++ = ReportBlock{k, j};
  }
}
static int block_section(const ReportBatch& B, const char* who, uint32_t* n_blocks, TableSection* out) {
  uint64_t n = 0;
  for (uint32_t k = 0; k < B.n_clouds; ++k) n += (B.cloud_points[k] + kReportBlockPoints - 1u) / kReportBlockPoints;
  if (n > 0x7fffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "%s: more than 2^31 blocks of 1024 points", who);
  *n_blocks = (uint32_t)n;
  *out = TableSection{(size_t)n * sizeof(ReportBlock), nullptr, fill_blocks, nullptr};
  return CLDN_HIP_OK;
}

// where the kernel writes the report: the caller's device report, or d_audit_rep for a HOST report ...
static int report_place(cldn_hip_codec* c, void* report, int report_loc, size_t rep_bytes, unsigned long long** d_rep) {
  *d_rep = (unsigned long long*)report;
  if (report_loc != CLDN_HIP_HOST) return CLDN_HIP_OK;
  const int rc = c->d_audit_rep.ensure(rep_bytes);
  *d_rep = (unsigned long long*)c->d_audit_rep.p;
  return rc;
}
// ... which then comes back: one copy, one synchronisation
static int report_fetch(cldn_hip_codec* c, void* report, int report_loc, const void* d_rep, size_t rep_bytes) {
  if (report_loc != CLDN_HIP_HOST) return CLDN_HIP_OK;
  HIP_TRY(hipMemcpyAsync(report, d_rep, rep_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return CLDN_HIP_OK;
}

// Host points of a *_clouds call go to d_audit at byte `at`; *d_ptr: where the kernel reads them. `room` is all that the call
// stages there (at + bytes <= room), the same in each of its uploads: the first sizes d_audit, a later one finds it large enough
// and moves nothing.
// (Pageable host buffers: a call with a DEVICE report synchronises before it returns, so that no copy still reads them; a HOST
// report has synchronised already.)
static int stage_host_points(cldn_hip_codec* c, const void* ptr, int loc, uint64_t bytes, size_t at, size_t room, const uint8_t** d_ptr) {
  *d_ptr = (const uint8_t*)ptr;
  if (loc != CLDN_HIP_HOST || bytes == 0) return CLDN_HIP_OK;
  const int rc = c->d_audit.ensure(room);
  if (rc != CLDN_HIP_OK) return rc;
  HIP_TRY(hipMemcpyAsync((uint8_t*)c->d_audit.p + at, ptr, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
  *d_ptr = (const uint8_t*)c->d_audit.p + at;
  return CLDN_HIP_OK;
}

// two device buffers -> report: tables up, one clear, one kernel; HOST report: one copy, one synchronisation
static int audit_device(cldn_hip_codec* c, const uint8_t* d_a, const uint8_t* d_b, const uint64_t* cloud_points, uint32_t n_clouds,
                        const std::vector<AuditField>& fields, cldn_hip_audit_field_t* report, int report_loc) {
  static_assert(sizeof(cldn_hip_audit_field_t) == 40, "five 64-bit words");
  const uint32_t n_fields = (uint32_t)fields.size();
  const size_t rep_bytes = (size_t)n_clouds * n_fields * sizeof(cldn_hip_audit_field_t);
  if (rep_bytes == 0) return CLDN_HIP_OK;
  int rc;
  AuditLaunch L;
  const ReportBatch B = {cloud_points, n_clouds, n_fields};
  TableSection sec[3] = {cloud_section(B), {}, field_section(fields)};
  if ((rc = block_section(B, "audit", &L.n_blocks, &sec[1])) != CLDN_HIP_OK) return rc;
  if ((rc = upload_tables(c, B, sec, 3)) != CLDN_HIP_OK) return rc;
  if ((rc = report_place(c, report, report_loc, rep_bytes, &L.report)) != CLDN_HIP_OK) return rc;
  L.stream = c->stream;
  L.a = d_a;
  L.b = d_b;
  L.point_step = c->plan.point_step;
  L.n_clouds = n_clouds;
  L.n_fields = n_fields;
  L.fields = fields.data();
  L.dev_fields = (const AuditField*)sec[2].dev;
  L.clouds = (const ReportCloud*)sec[0].dev;
  L.blocks = (const ReportBlock*)sec[1].dev;
  if ((rc = audit_launch(L)) != CLDN_HIP_OK) return rc;
  return report_fetch(c, report, report_loc, L.report, rep_bytes);
}

static int no_last_encode(const char* who) {
  return fail(CLDN_HIP_ERR_ARG, "%s: no encode call to audit (an encode call must be this codec's last call that touched buffers; "
                                "a chunk table must have been framed)", who);
}

static int audit_batch_points(const uint64_t* cloud_points, uint32_t n_clouds, uint64_t* total) {
  if (n_clouds && !cloud_points) return fail(CLDN_HIP_ERR_ARG, "cloud_points is NULL");
  uint64_t n = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) n += cloud_points[k];
  *total = n;
  return CLDN_HIP_OK;
}

// `points` against the decode of `streams`. d_audit: [host points | decode, zero-filled | host streams]
static int audit_streams_impl(cldn_hip_codec* c, const void* points, int points_loc, const void* streams, int streams_loc,
                              const uint64_t* stream_offsets, const uint64_t* cloud_points, uint32_t n_clouds, int stream_kind,
                              const double* limit, cldn_hip_audit_field_t* report, int report_loc) {
  if ((points_loc != CLDN_HIP_HOST && points_loc != CLDN_HIP_DEVICE) || (streams_loc != CLDN_HIP_HOST && streams_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (stream_kind != CLDN_HIP_STAGE2_NONE && stream_kind != CLDN_HIP_STAGE2_LZ4 && stream_kind != CLDN_HIP_STAGE2_ZSTD)
    return fail(CLDN_HIP_ERR_ARG, "audit_streams: stream_kind %d is neither framed stage-1 streams (0) nor LZ4 chunks (1) nor ZSTD chunks (%d)", stream_kind,
                (int)CLDN_HIP_STAGE2_ZSTD);
  int rc;
  if ((rc = report_check("audit", !c->plan.fields.empty(), n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<AuditField> fields;
  if ((rc = audit_fields(c->plan, limit, &fields)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = audit_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  if (n_clouds == 0) return CLDN_HIP_OK;
  if (!stream_offsets) return fail(CLDN_HIP_ERR_ARG, "NULL offsets / cloud_points");
  for (uint32_t k = 0; k < n_clouds; ++k)
    if (stream_offsets[k + 1] < stream_offsets[k]) return fail(CLDN_HIP_ERR_ARG, "stream_offsets must be ascending");
  if (n_points && !points) return fail(CLDN_HIP_ERR_ARG, "points is NULL");
  const uint64_t s0 = stream_offsets[0], s_bytes = stream_offsets[n_clouds] - s0;
  if (s_bytes && !streams) return fail(CLDN_HIP_ERR_ARG, "streams is NULL");
  ENTER_DEVICE(c->device);
  const uint64_t bytes = n_points * c->plan.point_step;
  const size_t pts_b = points_loc == CLDN_HIP_HOST ? ((size_t)bytes + 255u) & ~size_t(255) : 0u;
  const size_t dec_b = ((size_t)bytes + 255u) & ~size_t(255);
  const size_t str_b = streams_loc == CLDN_HIP_HOST ? (size_t)s_bytes : 0u;
  if ((rc = c->d_audit.ensure(std::max<size_t>(256, pts_b + dec_b + str_b))) != CLDN_HIP_OK) return rc;
  uint8_t* base = (uint8_t*)c->d_audit.p;
  const uint8_t* d_points = (const uint8_t*)points;
  if (points_loc == CLDN_HIP_HOST) {
    if (bytes) HIP_TRY(hipMemcpyAsync(base, points, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    d_points = base;
  }
  uint8_t* d_dec = base + pts_b;
  if (bytes) HIP_TRY(hipMemsetAsync(d_dec, 0, (size_t)bytes, c->stream));
  std::vector<uint64_t> rel(stream_offsets, stream_offsets + n_clouds + 1);
  for (uint64_t& o : rel) o -= s0;
  const uint8_t* d_streams = (const uint8_t*)streams + s0;
  if (streams_loc == CLDN_HIP_HOST) {
    if (s_bytes) HIP_TRY(hipMemcpyAsync(base + pts_b + dec_b, (const uint8_t*)streams + s0, (size_t)s_bytes, hipMemcpyHostToDevice, c->stream));
    d_streams = base + pts_b + dec_b;
  }
  if ((rc = decode_framed(c, d_streams, CLDN_HIP_DEVICE, rel.data(), cloud_points, n_clouds, nullptr, CLDN_HIP_HOST, d_dec, bytes,
                          CLDN_HIP_DEVICE, stream_kind)) != CLDN_HIP_OK)
    return rc;
  // the decode's verdict before the report is touched (also: the host buffers of this call have been read)
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->d_status.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((rc = decode_verdict(st)) != CLDN_HIP_OK) return rc;
  return audit_device(c, d_points, d_dec, cloud_points, n_clouds, fields, report, report_loc);
}

extern "C" {

int cldn_hip_audit_clouds(cldn_hip_codec_t* c, const void* a, int a_loc, const void* b, int b_loc, const uint64_t* cloud_points,
                          uint32_t n_clouds, const double* limit, cldn_hip_audit_field_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if ((a_loc != CLDN_HIP_HOST && a_loc != CLDN_HIP_DEVICE) || (b_loc != CLDN_HIP_HOST && b_loc != CLDN_HIP_DEVICE))
    return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  int rc;
  if ((rc = report_check("audit", !c->plan.fields.empty(), n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<AuditField> fields;
  if ((rc = audit_fields(c->plan, limit, &fields)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = audit_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  if (n_points && (!a || !b)) return fail(CLDN_HIP_ERR_ARG, "audit_clouds: NULL buffer");
  ENTER_DEVICE(c->device);
  const uint64_t bytes = n_points * c->plan.point_step;
  const size_t one = ((size_t)bytes + 255u) & ~size_t(255);
  const uint8_t *d_a, *d_b;
  const bool up_a = a_loc == CLDN_HIP_HOST && bytes, up_b = b_loc == CLDN_HIP_HOST && bytes;
  const size_t room = one * ((up_a ? 1u : 0u) + (up_b ? 1u : 0u));
  if ((rc = stage_host_points(c, a, a_loc, bytes, 0u, room, &d_a)) != CLDN_HIP_OK) return rc;
  if ((rc = stage_host_points(c, b, b_loc, bytes, up_a ? one : 0u, room, &d_b)) != CLDN_HIP_OK) return rc;
  rc = audit_device(c, d_a, d_b, cloud_points, n_clouds, fields, report, report_loc);
  if (rc == CLDN_HIP_OK && (up_a || up_b) && report_loc == CLDN_HIP_DEVICE) HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int cldn_hip_audit_streams(cldn_hip_codec_t* c, const void* points, int points_loc, const void* streams, int streams_loc,
                           const uint64_t* stream_offsets, const uint64_t* cloud_points, uint32_t n_clouds, int stream_kind,
                           const double* limit, cldn_hip_audit_field_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  return audit_streams_impl(c, points, points_loc, streams, streams_loc, stream_offsets, cloud_points, n_clouds, stream_kind, limit,
                            report, report_loc);
}

int64_t cldn_hip_audit_last_encode_clouds(const cldn_hip_codec_t* c) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->enc.valid) return no_last_encode("audit_last_encode");
  return (int64_t)c->enc.cloud_points.size();
}

int cldn_hip_audit_last_encode(cldn_hip_codec_t* c, const double* limit, cldn_hip_audit_field_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (cldn_hip_audit_last_encode_clouds(c) < 0) return CLDN_HIP_ERR_ARG;
  cldn_hip_codec::LastEncode E = c->enc;  // (the decode below drops the codec's copy)
  const cldn_hip_codec::LastEncode kept = c->enc;
  if (E.kind == CLDN_HIP_STAGE2_ZSTD) {  // the stage-1 streams of the call, still in the codec's workspace
    E.streams = E.s1_streams;
    E.d_offsets = E.d_s1_offsets;
    E.offsets.clear();
    E.kind = CLDN_HIP_STAGE2_NONE;
  }
  const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
  if (n_clouds == 0) return CLDN_HIP_OK;
  uint64_t n_points = 0;
  for (uint64_t n : E.cloud_points) n_points += n;
  if (n_points == 0) {  // nothing was launched and nothing written: empty streams
    E.streams = nullptr;
    E.offsets.assign((size_t)n_clouds + 1, 0);
  }
  if (E.offsets.empty()) {  // DEVICE outputs: the encode call has not read its offsets
    ENTER_DEVICE(c->device);
    E.offsets.resize((size_t)n_clouds + 1);
    HIP_TRY(hipMemcpyAsync(E.offsets.data(), E.d_offsets, ((size_t)n_clouds + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (E.offsets[k + 1] < E.offsets[k]) return fail(CLDN_HIP_ERR_DEVICE, "audit_last_encode: the encode call left no valid stream offsets (see cldn_hip_codec_status)");
  }
  const int rc = audit_streams_impl(c, E.points, CLDN_HIP_DEVICE, E.streams, CLDN_HIP_DEVICE, E.offsets.data(), E.cloud_points.data(),
                                    n_clouds, E.kind, limit, report, report_loc);
  c->enc = kept.kind == CLDN_HIP_STAGE2_ZSTD ? kept : E;
  return rc;
}

}  // extern "C"

// ---- resolution sweep: size and error per field and candidate (sweep_kernels.hip) ----

// the schema's fields and their ladders as the kernel wants them
static int sweep_tables(const cldn_hip_plan& P, const float* resolutions, uint32_t n_candidates, std::vector<SweepField>* fields,
                        std::vector<SweepCand>* cands) {
  if (n_candidates == 0 || n_candidates > CLDN_HIP_SWEEP_MAX_CANDIDATES)
    return fail(CLDN_HIP_ERR_ARG, "sweep: n_candidates is %u, must be 1..%u", n_candidates, CLDN_HIP_SWEEP_MAX_CANDIDATES);
  if (!P.fields.empty() && !resolutions) return fail(CLDN_HIP_ERR_ARG, "sweep: resolutions is NULL");
  fields->resize(P.fields.size());
  cands->assign(P.fields.size() * n_candidates, SweepCand{0.0, 0.0});
  for (size_t i = 0; i < P.fields.size(); ++i) {
    const cldn_hip_field_t& f = P.fields[i];
    SweepField& s = (*fields)[i];
    memset(&s, 0, sizeof(s));
    s.offset = f.offset;
    s.kind = SWEEP_NONE;
    if (P.encoding_opt != 1 || !f.has_resolution || (f.type != 7 && f.type != 8)) continue;
    const uint32_t op_kind = i < P.floatn_lanes ? OP_QF32 : (f.type == 7 ? OP_LOSSY_F32 : OP_LOSSY_F64);
    s.kind = op_kind == OP_QF32 ? SWEEP_QF32 : (op_kind == OP_LOSSY_F32 ? SWEEP_F32 : SWEEP_F64);
    if (f.offset == 0xffffffffu) return fail(CLDN_HIP_ERR_ARG, "sweep: field %zu is decoded but not stored (kDecodeButSkipStore)", i);
    for (uint32_t k = 0; k < n_candidates; ++k) {
      const float r = resolutions[i * n_candidates + k];
      if (r == 0.0f) continue;  // skip
      const float recip = 1.0F / r;
      if (!(r > 0.0f) || std::isinf(r) || recip == 0.0f || std::isinf(recip))
        return fail(CLDN_HIP_ERR_ARG, "sweep: resolution %u of field %zu (%g) must be 0 (skip) or positive and finite with a finite, non-zero float32 reciprocal",
                    k, i, (double)r);
      DevOp op;
      memset(&op, 0, sizeof(op));
      lossy_float_scale(op_kind, r, &op);
      SweepCand& C = (*cands)[i * n_candidates + k];
      C.m = op_kind == OP_LOSSY_F64 ? op.mult_d : (double)op.mult_f;
      C.r = op_kind == OP_LOSSY_F64 ? op.res_d : (double)op.res_f;
      if (!(C.m > 0.0) || std::isinf(C.m))
        return fail(CLDN_HIP_ERR_ARG, "sweep: resolution %u of field %zu (%g) has no usable multiplier", k, i, (double)r);
    }
  }
  return CLDN_HIP_OK;
}

// device points -> report: tables up, one clear, one kernel; HOST report: one copy, one synchronisation.
// hist: the report holds cldn_hip_hist_t (k_sweep_hist), else cldn_hip_sweep_cell_t (k_sweep)
static int sweep_device(cldn_hip_codec* c, const uint8_t* d_points, const uint64_t* cloud_points, uint32_t n_clouds,
                        const std::vector<SweepField>& fields, const std::vector<SweepCand>& cands, uint32_t n_candidates,
                        void* report, int report_loc, bool hist) {
  static_assert(sizeof(cldn_hip_sweep_cell_t) == 32, "four 64-bit words");
  static_assert(sizeof(cldn_hip_hist_t) == 2048, "256 64-bit words");
  const uint32_t n_fields = (uint32_t)fields.size();
  const size_t rep_bytes = (size_t)n_clouds * n_fields * n_candidates * (hist ? sizeof(cldn_hip_hist_t) : sizeof(cldn_hip_sweep_cell_t));
  if (rep_bytes == 0) return CLDN_HIP_OK;
  int rc;
  SweepLaunch L;
  const ReportBatch B = {cloud_points, n_clouds, n_fields};
  TableSection sec[4] = {cloud_section(B), {},
                         TableSection{cands.size() * sizeof(SweepCand), cands.data(), nullptr, nullptr}, field_section(fields)};
  if ((rc = block_section(B, "sweep", &L.n_blocks, &sec[1])) != CLDN_HIP_OK) return rc;
  if ((rc = upload_tables(c, B, sec, 4)) != CLDN_HIP_OK) return rc;
  if ((rc = report_place(c, report, report_loc, rep_bytes, &L.report)) != CLDN_HIP_OK) return rc;
  L.stream = c->stream;
  L.points = d_points;
  L.point_step = c->plan.point_step;
  L.n_clouds = n_clouds;
  L.n_fields = n_fields;
  L.n_candidates = n_candidates;
  L.fields = fields.data();
  L.dev_fields = (const SweepField*)sec[3].dev;
  L.cands = (const SweepCand*)sec[2].dev;
  L.clouds = (const ReportCloud*)sec[0].dev;
  L.blocks = (const ReportBlock*)sec[1].dev;
  if ((rc = hist ? sweep_hist_launch(L, c->hist_walk) : sweep_launch(L)) != CLDN_HIP_OK) return rc;
  return report_fetch(c, report, report_loc, L.report, rep_bytes);
}

// cldn_hip_sweep_clouds / cldn_hip_sweep_hist_clouds
static int sweep_clouds_impl(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points, uint32_t n_clouds,
                             const float* resolutions, uint32_t n_candidates, void* report, int report_loc, bool hist) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if (points_loc != CLDN_HIP_HOST && points_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  int rc;
  if ((rc = report_check("sweep", !c->plan.fields.empty(), n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<SweepField> fields;
  std::vector<SweepCand> cands;
  if ((rc = sweep_tables(c->plan, resolutions, n_candidates, &fields, &cands)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = audit_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  if (n_points && !points) return fail(CLDN_HIP_ERR_ARG, "sweep_clouds: points is NULL");
  ENTER_DEVICE(c->device);
  const uint64_t bytes = n_points * c->plan.point_step;
  const uint8_t* d_points;
  if ((rc = stage_host_points(c, points, points_loc, bytes, 0u, (size_t)bytes, &d_points)) != CLDN_HIP_OK) return rc;
  rc = sweep_device(c, d_points, cloud_points, n_clouds, fields, cands, n_candidates, report, report_loc, hist);
  if (rc == CLDN_HIP_OK && points_loc == CLDN_HIP_HOST && bytes && report_loc == CLDN_HIP_DEVICE) HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

// cldn_hip_sweep_last_encode / cldn_hip_sweep_hist_last_encode
static int sweep_last_encode_impl(cldn_hip_codec_t* c, const float* resolutions, uint32_t n_candidates, void* report, int report_loc,
                                  bool hist) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (cldn_hip_sweep_last_encode_clouds(c) < 0) return CLDN_HIP_ERR_ARG;
  const cldn_hip_codec::LastEncode& E = c->enc;  // read only: the state stays as it is
  const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
  int rc;
  if ((rc = report_check("sweep", !c->plan.fields.empty(), n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<SweepField> fields;
  std::vector<SweepCand> cands;
  if ((rc = sweep_tables(c->plan, resolutions, n_candidates, &fields, &cands)) != CLDN_HIP_OK) return rc;
  ENTER_DEVICE(c->device);
  return sweep_device(c, E.points, E.cloud_points.data(), n_clouds, fields, cands, n_candidates, report, report_loc, hist);
}

extern "C" {

int cldn_hip_sweep_clouds(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points, uint32_t n_clouds,
                          const float* resolutions, uint32_t n_candidates, cldn_hip_sweep_cell_t* report, int report_loc) {
  return sweep_clouds_impl(c, points, points_loc, cloud_points, n_clouds, resolutions, n_candidates, report, report_loc, false);
}

int64_t cldn_hip_sweep_last_encode_clouds(const cldn_hip_codec_t* c) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->enc.valid && !c->enc.await_frame) return no_last_encode("sweep_last_encode");  // (the points are there before the framing)
  return (int64_t)c->enc.cloud_points.size();
}

int cldn_hip_sweep_last_encode(cldn_hip_codec_t* c, const float* resolutions, uint32_t n_candidates, cldn_hip_sweep_cell_t* report,
                               int report_loc) {
  return sweep_last_encode_impl(c, resolutions, n_candidates, report, report_loc, false);
}

int cldn_hip_sweep_hist_clouds(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points, uint32_t n_clouds,
                               const float* resolutions, uint32_t n_candidates, cldn_hip_hist_t* report, int report_loc) {
  return sweep_clouds_impl(c, points, points_loc, cloud_points, n_clouds, resolutions, n_candidates, report, report_loc, true);
}

int cldn_hip_sweep_hist_last_encode(cldn_hip_codec_t* c, const float* resolutions, uint32_t n_candidates, cldn_hip_hist_t* report,
                                    int report_loc) {
  return sweep_last_encode_impl(c, resolutions, n_candidates, report, report_loc, true);
}

// Test and measurement hook, not part of the header: block-table entries a workgroup of k_sweep_hist walks (0 = kHistWalkBlocks).
// Reports never depend on it.
__attribute__((visibility("default"))) int cldn_hip_debug_hist_walk(cldn_hip_codec_t* c, uint32_t blocks) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->hist_walk = blocks;
  return CLDN_HIP_OK;
}

}  // extern "C"

// ---- histogram of the bytes of each cloud's stream (hist_kernels.hip) ----

// device streams -> report: the item table up, one clear, one kernel; HOST report: one copy, one synchronisation.
// offsets: HOST [n_clouds + 1], ascending, in bytes of d_streams
static int stream_hist_device(cldn_hip_codec* c, const uint8_t* d_streams, const uint64_t* offsets, uint32_t n_clouds,
                              cldn_hip_hist_t* report, int report_loc) {
  const size_t rep_bytes = (size_t)n_clouds * sizeof(cldn_hip_hist_t);
  if (rep_bytes == 0) return CLDN_HIP_OK;
  std::vector<StreamHistItem> items;
  for (uint32_t k = 0; k < n_clouds; ++k)
    for (uint64_t at = offsets[k]; at < offsets[k + 1]; at += kStreamHistItemBytes)
      items.push_back(StreamHistItem{at, std::min<uint64_t>(at + kStreamHistItemBytes, offsets[k + 1]), k, 0u});
  if (items.size() > 0x7fffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "stream_hist: more than 2^31 pieces of 128 KiB");
  int rc;
  StreamHistLaunch L;
  const ReportBatch B = {nullptr, n_clouds, 0u};
  TableSection sec[1] = {TableSection{items.size() * sizeof(StreamHistItem), items.data(), nullptr, nullptr}};
  if (!items.empty() && (rc = upload_tables(c, B, sec, 1)) != CLDN_HIP_OK) return rc;
  if ((rc = report_place(c, report, report_loc, rep_bytes, &L.report)) != CLDN_HIP_OK) return rc;
  L.stream = c->stream;
  L.streams = d_streams;
  L.n_clouds = n_clouds;
  L.n_items = (uint32_t)items.size();
  L.items = (const StreamHistItem*)sec[0].dev;
  if ((rc = stream_hist_launch(L)) != CLDN_HIP_OK) return rc;
  return report_fetch(c, report, report_loc, L.report, rep_bytes);
}

extern "C" {

int cldn_hip_stream_hist(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets, uint32_t n_clouds,
                         cldn_hip_hist_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if (streams_loc != CLDN_HIP_HOST && streams_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  int rc;
  if ((rc = report_check("stream_hist", true, n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  if (n_clouds == 0) return CLDN_HIP_OK;
  if (!stream_offsets) return fail(CLDN_HIP_ERR_ARG, "stream_hist: stream_offsets is NULL");
  for (uint32_t k = 0; k < n_clouds; ++k)
    if (stream_offsets[k + 1] < stream_offsets[k]) return fail(CLDN_HIP_ERR_ARG, "stream_offsets must be ascending");
  const uint64_t s0 = stream_offsets[0], s_bytes = stream_offsets[n_clouds] - s0;
  if (s_bytes && !streams) return fail(CLDN_HIP_ERR_ARG, "stream_hist: streams is NULL");
  ENTER_DEVICE(c->device);
  std::vector<uint64_t> rel(stream_offsets, stream_offsets + n_clouds + 1);
  for (uint64_t& o : rel) o -= s0;
  const uint8_t* d_streams;
  if ((rc = stage_host_points(c, (const uint8_t*)streams + s0, streams_loc, s_bytes, 0u, (size_t)s_bytes, &d_streams)) != CLDN_HIP_OK)
    return rc;
  rc = stream_hist_device(c, d_streams, rel.data(), n_clouds, report, report_loc);
  if (rc == CLDN_HIP_OK && streams_loc == CLDN_HIP_HOST && s_bytes && report_loc == CLDN_HIP_DEVICE) HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int cldn_hip_stream_hist_last_encode(cldn_hip_codec_t* c, cldn_hip_hist_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->enc.valid) return no_last_encode("stream_hist_last_encode");  // (a chunk table has no streams before its framing)
  if (c->enc.kind == CLDN_HIP_STAGE2_ZSTD) {
    // the stage-1 streams behind the frames, as the audit reads them: the histogram a ZSTD size is estimated from, and what
    // composes with cldn_hip_sweep_hist_*. (The offsets are read back per call: the kept ones describe the frames.)
    cldn_hip_codec::LastEncode E = c->enc;
    const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
    int rc;
    if ((rc = report_check("stream_hist", true, n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
    if (n_clouds == 0) return CLDN_HIP_OK;
    ENTER_DEVICE(c->device);
    uint64_t n_points = 0;
    for (uint64_t n : E.cloud_points) n_points += n;
    std::vector<uint64_t> offs((size_t)n_clouds + 1, 0);
    if (n_points == 0) return stream_hist_device(c, nullptr, offs.data(), n_clouds, report, report_loc);
    HIP_TRY(hipMemcpyAsync(offs.data(), E.d_s1_offsets, offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (offs[k + 1] < offs[k]) return fail(CLDN_HIP_ERR_DEVICE, "stream_hist_last_encode: the encode call left no valid stream offsets (see cldn_hip_codec_status)");
    return stream_hist_device(c, E.s1_streams, offs.data(), n_clouds, report, report_loc);
  }
  cldn_hip_codec::LastEncode& E = c->enc;
  const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
  int rc;
  if ((rc = report_check("stream_hist", true, n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  if (n_clouds == 0) return CLDN_HIP_OK;
  ENTER_DEVICE(c->device);
  uint64_t n_points = 0;
  for (uint64_t n : E.cloud_points) n_points += n;
  if (n_points == 0) {  // nothing was launched and nothing written: empty streams
    const std::vector<uint64_t> none((size_t)n_clouds + 1, 0);
    return stream_hist_device(c, nullptr, none.data(), n_clouds, report, report_loc);
  }
  if (E.offsets.empty()) {  // DEVICE outputs: the encode call has not read its offsets. Kept: the state describes the same call
    std::vector<uint64_t> offs((size_t)n_clouds + 1);
    HIP_TRY(hipMemcpyAsync(offs.data(), E.d_offsets, offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (offs[k + 1] < offs[k]) return fail(CLDN_HIP_ERR_DEVICE, "stream_hist_last_encode: the encode call left no valid stream offsets (see cldn_hip_codec_status)");
    E.offsets = offs;
  }
  return stream_hist_device(c, E.streams, E.offsets.data(), n_clouds, report, report_loc);
}

double cldn_hip_hist_entropy_bytes(const cldn_hip_hist_t* h) {
  if (!h) return 0.0;
  uint64_t n = 0;
  for (uint64_t v : h->bin) n += v;
  if (n == 0) return 0.0;
  double bits = 0.0;
  for (uint64_t v : h->bin)
    if (v) bits += (double)v * std::log2((double)n / (double)v);
  const double bytes = bits / 8.0;
  return bytes < (double)n ? bytes : (double)n;
}

}  // extern "C"

// ---- CRC-32 of each span of a byte buffer (crc_kernels.hip) ----

static int crc_check(const char* who, uint32_t n_spans, const void* crc, int crc_loc) {
  if (crc_loc != CLDN_HIP_HOST && crc_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  if (n_spans && !crc) return fail(CLDN_HIP_ERR_ARG, "%s: crc is NULL", who);
  if (crc_loc == CLDN_HIP_DEVICE && ((uintptr_t)crc & 3u)) return fail(CLDN_HIP_ERR_ARG, "%s: a device crc array must be 4-byte aligned", who);
  return CLDN_HIP_OK;
}

// device spans -> crc: the item table up, one clear, one kernel; HOST crc: one copy, one synchronisation.
// offsets: HOST [n_spans + 1], ascending, in bytes of d_streams. The items are cut where the kernel's lanes are: at the
// ADDRESSES that are multiples of kCrcSegmentBytes from the span's first 128-byte line. An item's multiplier is that of the
// item behind it times x^(8 * that item's length): one generic power per span (its last item), a constant for the others.
static int stream_crc32_device(cldn_hip_codec* c, const uint8_t* d_streams, const uint64_t* offsets, uint32_t n_spans, uint32_t* crc,
                               int crc_loc) {
  const size_t crc_bytes = (size_t)n_spans * sizeof(uint32_t);
  if (crc_bytes == 0) return CLDN_HIP_OK;
  static const CrcConstMul seg_pow(crc32_xpow8(kCrcSegmentBytes));  // (built once: 1024 multiplications)
  std::vector<CrcItem> items;
  for (uint32_t k = 0; k < n_spans; ++k) {
    if (offsets[k + 1] == offsets[k]) continue;
    const uintptr_t a = (uintptr_t)d_streams + offsets[k], e = (uintptr_t)d_streams + offsets[k + 1];
    const uintptr_t frame = a & ~(uintptr_t)(kCrcLaneBytes - 1u);
    const size_t first = items.size();
    for (uintptr_t at = frame; at < e; at += kCrcSegmentBytes) {
      const uintptr_t b = std::max(at, a), t = std::min<uintptr_t>(at + kCrcSegmentBytes, e);
      items.push_back(CrcItem{offsets[k] + (b - a), offsets[k] + (t - a), k, kCrcOne, at == frame ? 1u : 0u, 0u});
    }
    for (size_t j = items.size() - 1; j > first; --j)
      items[j - 1].mult = j + 1 == items.size() ? crc32_xpow8(items[j].end - items[j].begin) : seg_pow(items[j].mult);
  }
  // (one workgroup per item: HIP refuses a launch of 2^32 threads or more)
  if (items.size() > 0xffffffffull / kCrcThreads) return fail(CLDN_HIP_ERR_UNSUPPORTED, "stream_crc32: more than 2^24 pieces of 32 KiB");
  int rc;
  CrcLaunch L;
  const ReportBatch B = {nullptr, n_spans, 0u};
  TableSection sec[1] = {TableSection{items.size() * sizeof(CrcItem), items.data(), nullptr, nullptr}};
  if (!items.empty() && (rc = upload_tables(c, B, sec, 1)) != CLDN_HIP_OK) return rc;
  unsigned long long* d_crc;
  if ((rc = report_place(c, crc, crc_loc, crc_bytes, &d_crc)) != CLDN_HIP_OK) return rc;
  L.stream = c->stream;
  L.streams = d_streams;
  L.n_spans = n_spans;
  L.n_items = (uint32_t)items.size();
  L.items = (const CrcItem*)sec[0].dev;
  L.crc = (uint32_t*)d_crc;
  if ((rc = stream_crc32_launch(L)) != CLDN_HIP_OK) return rc;
  return report_fetch(c, crc, crc_loc, L.crc, crc_bytes);
}

extern "C" {

int cldn_hip_stream_crc32(cldn_hip_codec_t* c, const void* streams, int streams_loc, const uint64_t* stream_offsets, uint32_t n_streams,
                          uint32_t* crc, int crc_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if (streams_loc != CLDN_HIP_HOST && streams_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  int rc;
  if ((rc = crc_check("stream_crc32", n_streams, crc, crc_loc)) != CLDN_HIP_OK) return rc;
  if (n_streams == 0) return CLDN_HIP_OK;
  if (!stream_offsets) return fail(CLDN_HIP_ERR_ARG, "stream_crc32: stream_offsets is NULL");
  for (uint32_t k = 0; k < n_streams; ++k)
    if (stream_offsets[k + 1] < stream_offsets[k]) return fail(CLDN_HIP_ERR_ARG, "stream_offsets must be ascending");
  const uint64_t s0 = stream_offsets[0], s_bytes = stream_offsets[n_streams] - s0;
  if (s_bytes && !streams) return fail(CLDN_HIP_ERR_ARG, "stream_crc32: streams is NULL");
  ENTER_DEVICE(c->device);
  std::vector<uint64_t> rel(stream_offsets, stream_offsets + n_streams + 1);
  for (uint64_t& o : rel) o -= s0;
  const uint8_t* d_streams;
  if ((rc = stage_host_points(c, (const uint8_t*)streams + s0, streams_loc, s_bytes, 0u, (size_t)s_bytes, &d_streams)) != CLDN_HIP_OK)
    return rc;
  rc = stream_crc32_device(c, d_streams, rel.data(), n_streams, crc, crc_loc);
  if (rc == CLDN_HIP_OK && streams_loc == CLDN_HIP_HOST && s_bytes && crc_loc == CLDN_HIP_DEVICE) HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int cldn_hip_stream_crc32_last_encode(cldn_hip_codec_t* c, uint32_t* crc, uint64_t* sizes, int loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->enc.valid) return no_last_encode("stream_crc32_last_encode");  // (a chunk table has no streams before its framing)
  cldn_hip_codec::LastEncode& E = c->enc;  // the state stays; only the offsets of a DEVICE-output call are added to it
  const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
  int rc;
  if ((rc = crc_check("stream_crc32_last_encode", n_clouds, crc, loc)) != CLDN_HIP_OK) return rc;
  if (loc == CLDN_HIP_DEVICE && ((uintptr_t)sizes & 7u)) return fail(CLDN_HIP_ERR_ARG, "stream_crc32_last_encode: a device sizes array must be 8-byte aligned");
  if (n_clouds == 0) return CLDN_HIP_OK;
  ENTER_DEVICE(c->device);
  uint64_t n_points = 0;
  for (uint64_t n : E.cloud_points) n_points += n;
  // behind stage 2 on the device (LZ4 blocks, ZSTD frames): the stage-1 streams they were made from, still in the workspace
  const bool behind = E.kind != CLDN_HIP_STAGE2_NONE;
  const uint8_t* d_streams = behind ? E.s1_streams : E.streams;
  std::vector<uint64_t> read((size_t)n_clouds + 1, 0);
  const std::vector<uint64_t>* offs = &read;
  if (n_points == 0) {  // nothing was launched and nothing written: empty streams
    d_streams = nullptr;
  } else if (behind || E.offsets.empty()) {  // (DEVICE outputs: the encode call has not read its offsets)
    HIP_TRY(hipMemcpyAsync(read.data(), behind ? E.d_s1_offsets : E.d_offsets, read.size() * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_clouds; ++k)
      if (read[k + 1] < read[k]) return fail(CLDN_HIP_ERR_DEVICE, "stream_crc32_last_encode: the encode call left no valid stream offsets (see cldn_hip_codec_status)");
    if (!behind) E.offsets = read;  // kept: the state describes the same call
  } else {
    offs = &E.offsets;
  }
  const std::vector<uint64_t> o = *offs;  // (a copy: the call below may not touch the state, but the reference would alias it)
  if (sizes) {
    std::vector<uint64_t> s(n_clouds);
    for (uint32_t k = 0; k < n_clouds; ++k) s[k] = o[k + 1] - o[k];
    if (loc == CLDN_HIP_HOST) {
      memcpy(sizes, s.data(), s.size() * sizeof(uint64_t));
    } else {
      HIP_TRY(hipMemcpyAsync(sizes, s.data(), s.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // (a pageable source)
    }
  }
  return stream_crc32_device(c, d_streams, o.data(), n_clouds, crc, loc);
}

}  // extern "C"

// ---- sweep of the adaptive integer modes: section bytes per mode, probed and best mode (mode_kernels.hip) ----

static int modes_fields(const cldn_hip_plan& P, std::vector<ModeField>* out) {
  out->assign(P.adaptive_all.size(), ModeField{});
  for (size_t a = 0; a < P.adaptive_all.size(); ++a) {
    const DevAdaptive& d = P.adaptive_all[a];
    if ((d.bpv != 2u && d.bpv != 4u && d.bpv != 8u) || (uint64_t)d.offset + d.bpv > P.point_step)
      return fail(CLDN_HIP_ERR_ARG, "sweep_modes: adaptive field %zu (offset %u, %u bytes) exceeds point_step %u", a, d.offset,
                  (unsigned)d.bpv, P.point_step);
    ModeField& m = (*out)[a];
    m.offset = d.offset;
    m.type = d.type;
    m.bpv = d.bpv;
  }
  return CLDN_HIP_OK;
}

// The mode kernel's workgroups: chunks first, the probe last, field inner: the units of a chunk read the same points
static void fill_units(const ReportBatch& B, void* h) {
  ModeUnit* hu = (ModeUnit*)h;
  for (uint32_t k = 0; k < B.n_clouds; ++k) {
    const uint32_t nc = (uint32_t)((B.cloud_points[k] + kPointsPerChunk - 1u) / kPointsPerChunk);
    for (uint32_t j = 0; j < nc + (nc ? 1u : 0u); ++j)
      for (uint32_t a = 0; a < B.n_fields; ++a) *hu++ = ModeUnit{k, j < nc ? j : kModeProbeUnit, a, 0u};
  }
}

// device points -> report: tables up, one clear, one kernel; HOST report: one copy, one synchronisation
static int modes_device(cldn_hip_codec* c, const uint8_t* d_points, const uint64_t* cloud_points, uint32_t n_clouds,
                        const std::vector<ModeField>& fields, cldn_hip_mode_cell_t* report, int report_loc) {
  static_assert(sizeof(cldn_hip_mode_cell_t) == 40, "five 64-bit words");
  const uint32_t n_fields = (uint32_t)fields.size();
  const size_t rep_bytes = (size_t)n_clouds * n_fields * sizeof(cldn_hip_mode_cell_t);
  if (rep_bytes == 0) return CLDN_HIP_OK;
  int rc;
  uint64_t sections = 0;  // per field: the chunks of every cloud and one probe per cloud that has points
  for (uint32_t k = 0; k < n_clouds; ++k)
    sections += (cloud_points[k] + kPointsPerChunk - 1u) / kPointsPerChunk + (cloud_points[k] ? 1u : 0u);
  if (sections * n_fields > 0x7fffffffull) return fail(CLDN_HIP_ERR_UNSUPPORTED, "sweep_modes: more than 2^31 sections");
  ModeLaunch L;
  L.n_units = (uint32_t)(sections * n_fields);
  const ReportBatch B = {cloud_points, n_clouds, n_fields};
  TableSection sec[3] = {cloud_section(B), TableSection{(size_t)L.n_units * sizeof(ModeUnit), nullptr, fill_units, nullptr},
                         field_section(fields)};
  if ((rc = upload_tables(c, B, sec, 3)) != CLDN_HIP_OK) return rc;
  if ((rc = report_place(c, report, report_loc, rep_bytes, &L.report)) != CLDN_HIP_OK) return rc;
  L.stream = c->stream;
  L.points = d_points;
  L.point_step = c->plan.point_step;
  L.n_clouds = n_clouds;
  L.n_fields = n_fields;
  L.fields = fields.data();
  L.dev_fields = (const ModeField*)sec[2].dev;
  L.clouds = (const ReportCloud*)sec[0].dev;
  L.units = (const ModeUnit*)sec[1].dev;
  if ((rc = modes_launch(L)) != CLDN_HIP_OK) return rc;
  return report_fetch(c, report, report_loc, L.report, rep_bytes);
}

extern "C" {

int cldn_hip_sweep_modes_clouds(cldn_hip_codec_t* c, const void* points, int points_loc, const uint64_t* cloud_points,
                                uint32_t n_clouds, cldn_hip_mode_cell_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  c->enc.drop();
  if (points_loc != CLDN_HIP_HOST && points_loc != CLDN_HIP_DEVICE) return fail(CLDN_HIP_ERR_ARG, "invalid memory location tag");
  int rc;
  if ((rc = report_check("sweep_modes", c->plan.n_adaptive_total() != 0, n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<ModeField> fields;
  if ((rc = modes_fields(c->plan, &fields)) != CLDN_HIP_OK) return rc;
  uint64_t n_points = 0;
  if ((rc = audit_batch_points(cloud_points, n_clouds, &n_points)) != CLDN_HIP_OK) return rc;
  if (fields.empty()) return CLDN_HIP_OK;  // nothing to report
  if (n_points && !points) return fail(CLDN_HIP_ERR_ARG, "sweep_modes_clouds: points is NULL");
  ENTER_DEVICE(c->device);
  const uint64_t bytes = n_points * c->plan.point_step;
  const uint8_t* d_points;
  if ((rc = stage_host_points(c, points, points_loc, bytes, 0u, (size_t)bytes, &d_points)) != CLDN_HIP_OK) return rc;
  rc = modes_device(c, d_points, cloud_points, n_clouds, fields, report, report_loc);
  if (rc == CLDN_HIP_OK && points_loc == CLDN_HIP_HOST && bytes && report_loc == CLDN_HIP_DEVICE) HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

int cldn_hip_sweep_modes_last_encode(cldn_hip_codec_t* c, cldn_hip_mode_cell_t* report, int report_loc) {
  if (!c) return fail(CLDN_HIP_ERR_ARG, "codec is NULL");
  if (!c->enc.valid && !c->enc.await_frame) return no_last_encode("sweep_modes_last_encode");  // (the points are there before the framing)
  const cldn_hip_codec::LastEncode& E = c->enc;  // read only: the state stays as it is
  const uint32_t n_clouds = (uint32_t)E.cloud_points.size();
  int rc;
  if ((rc = report_check("sweep_modes", c->plan.n_adaptive_total() != 0, n_clouds, report, report_loc)) != CLDN_HIP_OK) return rc;
  std::vector<ModeField> fields;
  if ((rc = modes_fields(c->plan, &fields)) != CLDN_HIP_OK) return rc;
  if (fields.empty()) return CLDN_HIP_OK;
  ENTER_DEVICE(c->device);
  return modes_device(c, E.points, E.cloud_points.data(), n_clouds, fields, report, report_loc);
}

}  // extern "C"
