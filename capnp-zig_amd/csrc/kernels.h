// kernels.h — internal launcher interface between the C-ABI (capnp_packed_abi.cpp)
// and the gfx950 kernels (packed_kernels.hip and the headers under kernels/). Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "build_plan.h"
#include "capnp_packed.h"

namespace cpk {

// Batch encode / decode (write = false: sizes only). ws: optional caller workspace of
// at least queue_bytes(n) bytes for the batch's class workspace (class_ws.h; nullptr: the
// caller stream's own workspace, kept by the library).
hipError_t launch_encode(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                         uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                         int32_t* status, bool write, void* ws, size_t ws_bytes, hipStream_t stream);

hipError_t launch_decode(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                         uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                         int32_t* status, bool write, void* ws, size_t ws_bytes, hipStream_t stream);

size_t queue_bytes(uint32_t n);

// capnp_packed_set_decoder: returns the previous setting
int set_decoder(int decoder);
bool decoder_built(int decoder);  // AUTO, TWO_PASS, WORDS (FUSED / STREAM removed in round 5)
int set_all_or_nothing(int on);
uint32_t set_launch_flags(uint32_t flags);
hipError_t release_stream(hipStream_t stream, int dev = -1);  // dev -1: the current device
void stream_queue_info(hipStream_t stream, size_t* bytes, uint32_t* kept);
uint32_t stream_context_count();  // caller streams with a library context (current device)

// One unit (the single-buffer calls): the unit's status must be kStNeedFull (decode_one_status())
// for decode_one; encode_one takes units of at most 512 words.
int32_t decode_one_status();
hipError_t launch_decode_one(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                             const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                             hipStream_t stream);
hipError_t launch_encode_one(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out,
                             const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                             bool write, hipStream_t stream);
// Reader.readPackedMessage over a batch of reader streams (reader.zig:84-156).
hipError_t launch_read_message(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                               uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                               uint64_t* consumed, int32_t* status, hipStream_t stream);

// Resumable packed framing (capnp_packed_framer_*): batched device byte copies (3 u64 per job:
// dst, src, len), the header pass of Reader.readPackedMessage (framed length per unit), and the
// walk of each listed connection's message from its saved position.
hipError_t launch_copy_jobs(const uint64_t* jobs, uint32_t nj, hipStream_t stream);
hipError_t launch_read_header(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                              uint64_t* out_len, uint64_t* consumed, int32_t* status, hipStream_t stream);
// Framer walk (capnp_packed_framer_read): spec_q (framer_spec_bytes(nl, windows) bytes, the u64
// at u32 index kSlotReserved of class_ws.h = windows) holds the window tables of the listed connections whose held bytes
// span more than one window (spec_first / spec_count per list entry, spec_off / spec_len their
// bytes from the walk's start); spec_q null or windows 0: every window walked exactly.
size_t framer_spec_bytes(uint32_t nl, uint64_t windows);
uint32_t framer_window_bytes();            // the windows' size (kWvWin)
uint64_t framer_window_cap(uint32_t nl);   // windows a spec table of nl connections may hold
// The walk goes on message after message, up to M per connection: cnt[i] messages found, their
// packed and framed lengths at tab[2 (i M + m)] / [+ 1] (u32); need / X / W / status then hold
// the current message's state (frame_walk_kernel).
hipError_t launch_frame_walk(const uint8_t* arena, const uint32_t* list, uint32_t nl, const uint64_t* base,
                             const uint64_t* avail, uint64_t* need, uint64_t* X, uint64_t* W, int32_t* status,
                             uint32_t M, uint32_t* cnt, uint32_t* tab, uint32_t* spec_q, uint64_t windows,
                             const uint32_t* spec_first, const uint32_t* spec_count, const uint64_t* spec_off,
                             const uint64_t* spec_len, hipStream_t stream);

// Dense streams split into their packed messages (capnp_packed_split_streams):
// a wave per stream walks message after message, stateless. ws: at least
// split_workspace_bytes(n, 0) bytes, 256-B aligned, set up by a kernel on every call; what it
// holds beyond that is the window table (as many windows as fit, at most framer_window_cap(n)).
// max_msgs 0: counts, consumed and statuses only.
size_t split_workspace_bytes(uint32_t n, uint64_t in_bytes_bound);
hipError_t launch_split_streams(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                                uint64_t max_msgs, uint64_t* msg_first, uint64_t* msg_off, uint64_t* msg_len,
                                uint64_t* msg_framed, uint32_t* msg_stream, uint64_t* consumed, int32_t* status,
                                void* ws, size_t ws_bytes, hipStream_t stream);

// MessageBuilder.toPackedBytes from segment lists (message.zig:2123-2179).
hipError_t launch_encode_message(const uint64_t* seg_ptr, const uint64_t* seg_len, const uint32_t* seg_first,
                                 const uint32_t* seg_count, uint32_t n, uint8_t* out, const uint64_t* out_off,
                                 const uint64_t* out_cap, uint64_t* out_len, int32_t* status, bool write,
                                 hipStream_t stream);

// The C++ dialect (CAPNP_PACKED_DIALECT_CXX) of launch_encode / launch_encode_message: a wave per
// unit / message in one kernel; no workspace, no side stream.
hipError_t launch_encode_cxx(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                             uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                             int32_t* status, bool write, hipStream_t stream);
hipError_t launch_encode_message_cxx(const uint64_t* seg_ptr, const uint64_t* seg_len, const uint32_t* seg_first,
                                     const uint32_t* seg_count, uint32_t n, uint8_t* out, const uint64_t* out_off,
                                     const uint64_t* out_cap, uint64_t* out_len, int32_t* status, bool write,
                                     hipStream_t stream);

// MessageBuilder.writePackedTo unit after unit on one writer (message.zig:2209-2213): the batch
// packed into ONE dense stream out[out_base ..) in unit order, out_off[i] / out_off[n] the
// running offsets, in one pass over the input (encode_dense_kernel: an ordered single-pass
// prefix over tiles of units with decoupled look-back). out null: sizes and
// offsets only. ws: dense_workspace_bytes(n) bytes, 256-B aligned, zeroed here on every call.
size_t dense_workspace_bytes(uint32_t n);
hipError_t launch_encode_dense(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                               uint8_t* out, uint64_t out_base, uint64_t out_cap, uint64_t* out_off,
                               uint64_t* out_len, int32_t* status, bool cxx, bool framed, void* ws,
                               hipStream_t stream);

// Framed messages as units (capnp_packed_encode_framed_*): launch_encode_dense's
// `framed` above, and the slot call here. Each unit is checked as Message.init checks it, plus
// the exact-length rule; under the C++ dialect its segment table and segments are packed piece
// by piece. ws: framed_workspace_bytes(n) bytes, 256-B aligned (the Zig dialect's; the C++
// dialect takes none).
size_t framed_workspace_bytes(uint32_t n);
hipError_t launch_encode_framed(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                                uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                                int32_t* status, bool write, bool cxx, void* ws, hipStream_t stream);

// Message.init segment-table parse (message.zig:341-394).
hipError_t launch_message_init(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                               uint32_t max_segs, uint32_t* seg_count, uint64_t* seg_off, uint64_t* seg_len,
                               int32_t* status, hipStream_t stream);

// Message.validate (message.zig:699-969) of framed messages.
hipError_t launch_validate(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                           uint64_t seg_limit, uint64_t trav_limit, uint32_t nest_limit, int32_t* status,
                           uint64_t* words, hipStream_t stream);

// StructReader's reads over a batch (capnp_packed_read_fields_batch): the
// descriptors (host memory, checked by the caller, at most CAPNP_PACKED_MAX_FIELDS) go to the
// kernel by value. launch_gather: the ragged byte copy of capnp_packed_gather_batch.
hipError_t launch_read_fields(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                              const capnp_packed_field* fields, uint32_t n_fields, uint64_t* value, uint64_t* len,
                              uint64_t* count, int32_t* status, hipStream_t stream);
hipError_t launch_gather(const uint8_t* in, const uint64_t* src_off, const uint64_t* src_len, uint32_t n,
                         uint8_t* out, const uint64_t* dst_off, uint64_t out_cap, int32_t* status,
                         hipStream_t stream);

// Struct lists and pointer lists as element tables (capnp_packed_list_heads_batch and
// capnp_packed_read_elements_batch): `path` (at most CAPNP_PACKED_MAX_PATH) and
// `fields` are host memory, checked by the caller, and go to the kernels by value; the grid of
// launch_read_elements is sized from elem_cap (below 2^32, above 0).
hipError_t launch_list_heads(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                             const uint32_t* path, uint32_t path_len, uint32_t pointer_index, uint32_t list_kind,
                             capnp_packed_list_head* head, uint64_t* count, int32_t* status, hipStream_t stream);
hipError_t launch_read_elements(const uint8_t* in, const uint64_t* in_off, uint32_t n,
                                const capnp_packed_list_head* head, const uint64_t* elem_start, uint32_t list_kind,
                                uint64_t elem_cap, const capnp_packed_field* fields, uint32_t n_fields,
                                uint32_t* parent, uint32_t* index, uint64_t* value, uint64_t* len, uint64_t* count,
                                int32_t* status, hipStream_t stream);

// MessageBuilder / StructBuilder over a batch (capnp_packed_build_fields_batch):
// the plan (build_plan.h's sb_compile, which is the caller's check of the ops) goes to the kernel
// by value; out == nullptr gives lengths and statuses only.
hipError_t launch_build_fields(const uint8_t* pool, uint64_t pool_len, uint32_t n, const SbPlan& plan,
                               const uint64_t* value, const uint64_t* len, const uint64_t* count, uint8_t* out,
                               const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                               hipStream_t stream);

hipError_t launch_generate(uint8_t* out, uint64_t n_units, uint64_t unit_bytes, uint64_t unit_base,
                           uint64_t seed, uint32_t thr, hipStream_t stream);

size_t scan_scratch_bytes(uint32_t n);

hipError_t launch_scan(const uint64_t* len, uint32_t n, uint64_t base, uint64_t* off, uint64_t* scratch,
                       hipStream_t stream);

}  // namespace cpk
