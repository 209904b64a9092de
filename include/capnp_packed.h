/*
 * capnp_packed.h — C-ABI of the MI355X-native Cap'n Proto *packed* codec.
 *
 * This is the drop-in boundary for the reference's packed read/write surface
 * (nullstyle/capnp-zig, src/serialization/message.zig). Every entry point below
 * names the reference function it replaces. The reference functions are
 * file-private Zig functions; INTEGRATION.md shows the `extern fn` binding and the
 * three-line patch a maintainer applies to message.zig to route them here.
 *
 * Signatures use plain pointers, sizes and an opaque stream handle only.
 *
 * Codec rules are the Zig rules by default (NOT canonical C++ capnp): see DESIGN.md §1. The
 * capnp_packed_encode_*_dialect calls write the C++ capnp / pycapnp bytes on request
 * (CAPNP_PACKED_DIALECT_CXX); every decoder reads both.
 *
 * Ownership: the caller owns every buffer. Output capacity is passed in; the
 * library never allocates caller-visible memory. A Zig caller allocates
 * `capnp_packed_encode_bound(n)` (or the size from `capnp_packed_decoded_size`)
 * and shrinks with `allocator.realloc`, which keeps Zig's exact-length free
 * contract (message.zig:144/270 `toOwnedSlice`).
 *
 * Threading: all functions are thread-safe. The single-buffer host functions
 * serialise on one internal device context. One-time device init is guarded by
 * std::call_once. Batch functions keep per-(device, caller stream) state only:
 * encode/encoded_size/decode batches put their long units (more than 4 KiB in;
 * packed units beyond the fast decoder's window) on a side stream of THAT caller
 * stream, forked from and joined back into `stream` inside the call, so ordering
 * on `stream` is as if everything ran on it and batches on different caller
 * streams never wait on each other.
 */
#ifndef CAPNP_PACKED_H
#define CAPNP_PACKED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version (INTEGRATION.md §5 lists what changed):
 *   2 (round 5): capnp_packed_framer_* and capnp_packed_set_launch_flags (added in round 4),
 *     capnp_packed_stream_contexts, CAPNP_PACKED_DECODER_WORDS; CAPNP_PACKED_DECODER_FUSED /
 *     _STREAM answer INVALID_ARGUMENT (those decoders were removed from the library in round 5,
 *     source at 869fccf), and the CPK_DECODE environment variable is gone
 *     (capnp_packed_set_decoder is the only selector). Round 6 changed no signature.
 *   2, additions only: CAPNP_PACKED_DIALECT_ZIG / _CXX and capnp_packed_encode_dialect,
 *     capnp_packed_encode_batch_dialect, capnp_packed_encode_message_batch_dialect (the opt-in
 *     C++-canonical encoder). Nothing that existed changed.
 *   2, additions only: capnp_packed_encode_dense_workspace_bytes and
 *     capnp_packed_encode_dense_batch (the batch form of writePackedTo).
 *   2, additions only: capnp_packed_split_workspace_bytes and capnp_packed_split_streams (dense
 *     streams of packed messages split into their messages: the reader's half of the above).
 *   2, additions only: capnp_packed_encode_framed, capnp_packed_encode_framed_workspace_bytes,
 *     capnp_packed_encode_framed_batch and capnp_packed_encode_framed_dense_batch (the encoders
 *     over framed messages: under DIALECT_CXX the bytes of capnp convert binary:packed).
 *   2, additions only: capnp_packed_read_fields_batch, capnp_packed_gather_batch, the
 *     capnp_packed_field descriptor and the CAPNP_PACKED_FIELD_* kinds (the root struct's and
 *     nested structs' scalar and slice reads as columns, and the slices as dense bytes).
 *   2, additions only: capnp_packed_list_heads_batch, capnp_packed_read_elements_batch, the
 *     capnp_packed_list_head record and the CAPNP_PACKED_LIST_* kinds (struct lists and pointer
 *     lists as element tables).
 *   2, additions only: capnp_packed_build_fields_batch, the capnp_packed_build_op descriptor and
 *     the CAPNP_PACKED_BUILD_* constants (single-segment struct building over a batch: columns to
 *     framed messages). */
#define CAPNP_PACKED_ABI_VERSION 2u

/* Status codes. The first four mirror the reference's error set
 * (message.zig:201 InvalidMessageSize, :105/:115/:121/:127/:137 UnexpectedEof,
 * :163/:168 Overflow, allocator OutOfMemory -> OUT_OF_SPACE because the caller
 * supplies capacity). */
enum capnp_packed_status {
    CAPNP_PACKED_OK = 0,
    CAPNP_PACKED_INVALID_MESSAGE_SIZE = 1, /* encode input length % 8 != 0 (message.zig:201) */
    CAPNP_PACKED_UNEXPECTED_EOF = 2,       /* truncated packed input (message.zig:152-191) */
    CAPNP_PACKED_OVERFLOW = 3,             /* decoded size overflows size_t (message.zig:163); unreachable for < 2^60-byte inputs */
    CAPNP_PACKED_OUT_OF_SPACE = 4,         /* output capacity too small; *out_len holds the required size */
    CAPNP_PACKED_INVALID_ARGUMENT = 5,     /* null pointer, decreasing offsets, or a misaligned word-side offset */
    CAPNP_PACKED_DEVICE_ERROR = 6,         /* HIP runtime error; see capnp_packed_last_error() */
    CAPNP_PACKED_NO_DEVICE = 7,            /* no gfx950 device / HIP code object not loadable */
    /* Reader.readPackedMessage (reader.zig:84-156) only: */
    CAPNP_PACKED_END_OF_STREAM = 8,             /* the stream ends inside the message (readByte/readNoEof) */
    CAPNP_PACKED_INVALID_SEGMENT_COUNT = 9,     /* segment count - 1 == 0xFFFFFFFF (reader.zig:123) */
    CAPNP_PACKED_SEGMENT_COUNT_LIMIT_EXCEEDED = 10, /* more than 512 segments (reader.zig:125) */
    CAPNP_PACKED_MESSAGE_TOO_LARGE = 11,        /* more than 8 Mi words (reader.zig:140) */
    CAPNP_PACKED_INVALID_PACKED_MESSAGE = 12,   /* the last record overshoots the framed length (reader.zig:151-153) */
    /* Message.init (message.zig:341-394) only: */
    CAPNP_PACKED_TRUNCATED_MESSAGE = 13,        /* header or a segment runs past the data (message.zig:353/380) */
    /* Message.validate (message.zig:699-969) only: */
    CAPNP_PACKED_EMPTY_MESSAGE = 14,            /* no segments (:700) */
    CAPNP_PACKED_NESTING_LIMIT_EXCEEDED = 15,   /* a non-null pointer past the nesting limit (:724) */
    CAPNP_PACKED_INVALID_SEGMENT_ID = 16,       /* a pointer or landing pad names a missing segment (:421/:431/:725/:761) */
    CAPNP_PACKED_INVALID_POINTER = 17,          /* pointer type 3 (capability) where data is validated (:732) */
    CAPNP_PACKED_OUT_OF_BOUNDS = 18,            /* an object runs past its segment (bounds.zig:10-13) */
    CAPNP_PACKED_TRAVERSAL_LIMIT_EXCEEDED = 19, /* more words than traversal_limit_words (:711) */
    CAPNP_PACKED_INVALID_FAR_POINTER = 20,      /* malformed double-far landing pad (:758-760, :771) */
    CAPNP_PACKED_INVALID_INLINE_COMPOSITE_POINTER = 21, /* bad inline-composite tag (:585-596, :835-845, :938) */
    CAPNP_PACKED_LIST_TOO_LARGE = 22            /* list size overflows (:945; unreachable: sizes < 2^46 words) */
};

/* Version / capability query (precedent: src/wasm/capnp_host_abi.zig:60-70). */
uint32_t capnp_packed_abi_version(void);

/* Message of the last failing call on this thread (precedent:
 * capnp_host_abi.zig:165-184 last-error). Never NULL. */
const char* capnp_packed_last_error(void);

/* Name of a status code, e.g. "UnexpectedEof" (the reference's error names). */
const char* capnp_packed_status_name(int status);

/* Upper bound on the packed size of an n-byte input: 10 * (n / 8).
 * Replaces the implicit growth of std.ArrayList in packPacked (message.zig:204-270). */
size_t capnp_packed_encode_bound(size_t n);

/* ------------------------------------------------------------------------
 * Single-buffer functions on HOST memory (one unit through the GPU).
 * ------------------------------------------------------------------------ */

/* Replaces `fn packPacked(allocator, bytes) ![]u8` (message.zig:200-271).
 * Writes the packed bytes to out[0..*out_len). On OUT_OF_SPACE, *out_len is the
 * required size and out is untouched. */
int capnp_packed_encode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);

/* Replaces `fn estimateUnpackedSize(packed) !usize` (message.zig:152-191). */
int capnp_packed_decoded_size(const uint8_t* in, size_t n, size_t* out_size);

/* Replaces `fn unpackPacked(allocator, packed) ![]u8` (message.zig:88-145).
 * One host-to-device copy and one device decode into a device slot of min(cap, 8 n,
 * at least 64 KiB) bytes; if the unit needs more and cap holds it, the decode runs again
 * from the input already on the device into a slot of exactly that size. The output is
 * copied back only when the unit is OK, so errors are raised before any output byte
 * reaches `out`, as in the reference (size pass first), and out is untouched on any
 * error. On OUT_OF_SPACE, *out_len is the required size: a caller may pass a guessed
 * capacity and call again with the exact one. The device buffers grow with the largest
 * call and are given back by the next call needing a quarter of them or less (> 64 MiB). */
int capnp_packed_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);

/* ------------------------------------------------------------------------
 * Batch functions on DEVICE memory (the hot path).
 *
 * A batch is n independent units. Unit i's input is
 *   d_in[d_in_off[i] .. d_in_off[i] + d_in_len[i])
 * and its output goes to the capacity slot
 *   d_out[d_out_off[i] .. d_out_off[i] + d_out_cap[i])
 * d_out_len[i] receives the produced (or, on OUT_OF_SPACE, required) length and
 * d_status[i] the unit's status. All arrays have n entries and live in device
 * memory; offsets/lengths are u64 bytes. Because lengths are separate arrays,
 * an encode's d_out_off/d_out_len can be passed unchanged as a decode's
 * d_in_off/d_in_len (decode straight from the capacity slots), and dense
 * streams come from capnp_packed_lengths_to_offsets.
 *
 * Word-side alignment: the unpacked side of every unit (encode input, decode
 * output) must start at a multiple of 8 bytes (INVALID_ARGUMENT otherwise); the
 * packed side may start anywhere (dense packed streams are supported). An empty encode
 * unit whose input offset is misaligned is INVALID_ARGUMENT too (out_len 0, nothing
 * written), while an empty decode unit is OK whatever its slot's alignment.
 *
 * `stream` is a hipStream_t (NULL = default stream). Calls are asynchronous:
 * they enqueue kernels and return. The return value reports launch errors only;
 * per-unit results are in d_status / d_out_len. A unit that fails never has a byte
 * written past its out_cap, or outside its slot. Inside the slot, at every batch size,
 * the default contract is: the content of a failed decode unit's [0, out_cap) is
 * unspecified (the streaming kernels, for small units and for the words decoder's mid
 * units, may leave a prefix of its output), and likewise for an encode unit that ends
 * OUT_OF_SPACE. capnp_packed_set_all_or_nothing(1) makes every failed decode unit leave
 * its slot untouched, as unpackPacked does (message.zig:88-145 returns the error before
 * any output); or run capnp_packed_decoded_size_batch first.
 *
 * Workspace: encode / encoded_size / decode batches need a class workspace of
 * capnp_packed_batch_workspace_bytes(n) bytes (~750 B per unit + ~6 MiB: the small / mid /
 * long unit lists, the per-block class counts, the long-unit tile / window table, and
 * 704 B per unit of piece records for the indexed decoder, kept out of the caller's
 * output slots). The plain calls
 * use a queue the library keeps per caller stream (made on the first batch, grown to at
 * least twice its size on a batch larger than it holds; growing is refused with
 * DEVICE_ERROR inside a hipGraph capture). A replaced queue is freed once the stream has
 * drained, unless a capture used it: graphs that captured it stay valid, and it is kept
 * until capnp_packed_stream_release. The *_ws calls take the caller's device workspace
 * instead (256-B aligned, as hipMalloc returns; INVALID_ARGUMENT otherwise): nothing
 * of the library's is captured, and a graph of them may replay beside any work.
 * ------------------------------------------------------------------------ */

/* Batch packPacked (message.zig:200-271), one unit = one packPacked call. */
int capnp_packed_encode_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                              uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                              const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                              void* stream);

/* Bytes of device workspace the *_batch_ws calls need for n units. */
size_t capnp_packed_batch_workspace_bytes(uint32_t n);

/* Free what the library keeps for a caller stream (its side stream, events and queues,
 * also queues a captured graph used). Call after the stream's work is done, before the
 * stream is destroyed, and only when no graph captured from it will replay again. The
 * next batch on the stream starts a new context. Synchronises the stream. */
int capnp_packed_stream_release(void* stream);

/* The queue the library holds for a caller stream: its size in bytes (0: none) and how
 * many replaced queues it keeps because a hipGraph capture used them. */
int capnp_packed_stream_queue_info(void* stream, size_t* bytes, uint32_t* kept);

/* How many caller streams the library holds a context for (on the current device): a leak
 * check. A framer session's own stream is released with the session (round 5). */
int capnp_packed_stream_contexts(uint32_t* count);

/* capnp_packed_encode_batch with a caller-owned device workspace of at least
 * capnp_packed_batch_workspace_bytes(n) bytes (NULL = the library's per-stream
 * queue). The workspace must not be used by another batch in flight. */
int capnp_packed_encode_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                 uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                 const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* Packed sizes only (no output written): the first half of a dense encode
 * (sizes -> exclusive scan -> capnp_packed_encode_batch with dense offsets). */
int capnp_packed_encoded_size_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint64_t* d_out_len, int32_t* d_status, void* stream);

/* Batch unpackPacked (message.zig:88-145). */
int capnp_packed_decode_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                              uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                              const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                              void* stream);

/* capnp_packed_decode_batch with a caller-owned device workspace (as
 * capnp_packed_encode_batch_ws). */
int capnp_packed_decode_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                 uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                 const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* Batch estimateUnpackedSize (message.zig:152-191). */
int capnp_packed_decoded_size_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint64_t* d_out_len, int32_t* d_status, void* stream);

/* Batch Reader.readPackedMessage (reader.zig:84-156). Unit i is the buffered
 * packed byte stream of one reader (e.g. one connection). ONE message is decoded
 * from its front, stopping at the framed length its segment table declares; the
 * bytes after it (the next message) are not read.
 *   d_out_len[i]  framed (unpacked) bytes written to the slot
 *   d_consumed[i] packed bytes the message took: the caller advances the reader
 *                 by it and calls again for the next message
 * Per-unit errors leave d_consumed = 0 and d_out_len = 0:
 *   END_OF_STREAM (the message is incomplete: call again with more bytes),
 *   INVALID_SEGMENT_COUNT, SEGMENT_COUNT_LIMIT_EXCEEDED, MESSAGE_TOO_LARGE,
 *   INVALID_PACKED_MESSAGE (the last record overshoots the framed length).
 * OUT_OF_SPACE instead reports the framed length in d_out_len and the message's
 * packed length in d_consumed (retry with a larger slot). */
int capnp_packed_read_message_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                    const uint64_t* d_out_cap, uint64_t* d_out_len, uint64_t* d_consumed,
                                    int32_t* d_status, void* stream);

/* Connection.handleRead (src/rpc/level2/connection.zig:153-203) over n connections at
 * once, with the Framer's popFrame (src/rpc/level0/framing.zig:4-90) as
 * Reader.readPackedMessage on the device: a native host loop, HOST memory in and out.
 * Connection c's buffered bytes are in[in_off[c] .. +in_len[c]) of in[0..in_bytes).
 * One H2D of the input, then rounds of the batched reader (one unit per connection
 * that may still hold a message); each round's frames are copied D2H straight into
 * `frames`, so frame i is frames[frame_off[i] .. +frame_len[i]) of connection
 * frame_conn[i] (frames of a connection in order; *n_frames of them).
 * slot_guess[c] (in/out): the device slot for c's next frame (its last frame's size;
 *   a round that reports OUT_OF_SPACE is redone for c with the framed length).
 * consumed[c]: packed bytes of c's popped frames (the caller drops them from its buffer).
 * status[c]: END_OF_STREAM when c's bytes end inside a message or are used up (the rest
 *   waits for the next read: popFrame's null), else the reader's error that closes c
 *   (frames popped before it are still listed).
 * Returns OUT_OF_SPACE when `frames` (frames_cap bytes) or the frame table (max_frames)
 * is too small: nothing is valid then; retry with larger ones. */
int capnp_packed_frame_connections(const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                                   const uint64_t* in_len, uint32_t n, uint64_t* slot_guess, uint8_t* frames,
                                   uint64_t frames_cap, uint64_t* frame_off, uint64_t* frame_len,
                                   uint32_t* frame_conn, uint32_t max_frames, uint64_t* consumed, int32_t* status,
                                   uint32_t* n_frames);

/* Resumable framing of packed socket streams: Connection.handleRead
 * (src/rpc/level2/connection.zig:153-203) over n connections whose Framer state lives on the
 * device between reads (src/rpc/level0/framing.zig:42-90 keeps expected_total across pushes;
 * Reader.readPackedMessage, reader.zig:84-156, is one pass). A session keeps each connection's
 * unconsumed packed bytes in device memory, the current message's framed length once its
 * header is decoded, and where the walk to its end stopped: a read uploads only its new bytes
 * and the walk resumes there, so a message split over k reads is uploaded once and walked
 * once. A session is used by one thread at a time (calls serialise on it). */
typedef struct capnp_packed_framer capnp_packed_framer;
int capnp_packed_framer_create(uint32_t n_conns, capnp_packed_framer** out);
int capnp_packed_framer_destroy(capnp_packed_framer* f);
/* Append the new reads and pop every whole message. Connection c's new bytes are
 * in[in_off[c] .. +in_len[c]) of in[0..in_bytes) (in_len[c] = 0: none; in_off / in_len may be
 * NULL when in_bytes is 0). Frames as capnp_packed_frame_connections: frame i is
 * frames[frame_off[i] .. +frame_len[i]) of connection frame_conn[i], a connection's frames in
 * order. status[c] (n entries): END_OF_STREAM (its bytes end inside a message or are used up:
 * popFrame's null), or the reader's error, after which the connection's bytes are dropped (the
 * reset handleRead does, connection.zig:175-184; frames popped before it are listed).
 * OUT_OF_SPACE: `frames` or the frame table filled up; the listed frames are valid and popped,
 * the other whole messages stay buffered: call again (in_bytes = 0) to pop them.
 * One walk pass finds every whole message a connection holds (up to 64 per pass), one decode
 * pass frames them all; page-locked `in` and `frames` let the copies run at the link's rate. */
int capnp_packed_framer_read(capnp_packed_framer* f, const uint8_t* in, uint64_t in_bytes, const uint64_t* in_off,
                             const uint64_t* in_len, uint8_t* frames, uint64_t frames_cap, uint64_t* frame_off,
                             uint64_t* frame_len, uint32_t* frame_conn, uint32_t max_frames, int32_t* status,
                             uint32_t* n_frames);
/* capnp_packed_framer_read over the connections' own buffers (the reference keeps one
 * Framer.buffer per connection, framing.zig:6-8): connection c's new bytes are
 * in_ptr[c][0 .. in_len[c]) (in_len[c] = 0: none, in_ptr[c] may then be NULL). The library
 * gathers them into a page-locked staging buffer of the session (by byte range over up to 8
 * threads from 4 MiB up) and uploads that; no caller-side layout or pinning is needed. Frames,
 * status and OUT_OF_SPACE as capnp_packed_framer_read (call that, with in_bytes = 0, to pop the
 * rest). */
int capnp_packed_framer_readv(capnp_packed_framer* f, const uint8_t* const* in_ptr, const uint64_t* in_len,
                              uint8_t* frames, uint64_t frames_cap, uint64_t* frame_off, uint64_t* frame_len,
                              uint32_t* frame_conn, uint32_t max_frames, int32_t* status, uint32_t* n_frames);
/* Framer.reset (framing.zig:34-37) of one connection: its buffered bytes and state dropped. */
int capnp_packed_framer_reset(capnp_packed_framer* f, uint32_t conn);
/* Framer.bufferedBytes (framing.zig:30-32): packed bytes held for the connection. */
int capnp_packed_framer_buffered(capnp_packed_framer* f, uint32_t conn, uint64_t* bytes);
/* Framer.expected_total (framing.zig:10, :89): framed bytes of the connection's current message
 * once its header has been decoded, else 0. After OUT_OF_SPACE from capnp_packed_framer_read,
 * a frames buffer of the largest such size (rounded up to 8) pops that message. */
int capnp_packed_framer_expected(capnp_packed_framer* f, uint32_t conn, uint64_t* framed_bytes);
/* Bytes copied host-to-device (every read's bytes once) and moved between device regions since
 * the session was made (a connection's bytes move when its region doubles). */
int capnp_packed_framer_stats(capnp_packed_framer* f, uint64_t* uploaded, uint64_t* moved);
/* Walk passes run since the session was made (a call of capnp_packed_framer_read / _readv, with
 * or without new bytes, runs one per 64 messages of the connection with the most to walk, and none
 * when no connection holds bytes) and the windows those passes built lookup tables for: 0 while
 * every walk went window by window. Host-side counters, for tests and tuning. */
int capnp_packed_framer_walk_stats(capnp_packed_framer* f, uint64_t* passes, uint64_t* table_windows);

/* Single-buffer Reader.readPackedMessage on HOST memory: decodes the message at
 * the front of in[0..n) into out[0..*out_len); *consumed = packed bytes used.
 * On OUT_OF_SPACE, *out_len is the framed length. */
int capnp_packed_read_message(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                              size_t* consumed);

/* MessageBuilder.toPackedBytes (message.zig:2175-2179 = packPacked(toBytes()),
 * toBytes 2123-2170) for n messages, packed straight from their segments: the
 * framed bytes (segment table + segments) are never materialised. Message i has
 * d_seg_count[i] segments (0 = one empty segment, as toBytes adds one) listed
 * from index d_seg_first[i] of d_seg_ptr (device addresses, 8-byte aligned) and
 * d_seg_len (bytes, multiples of 8, as a MessageBuilder's segments are). At most
 * 512 segments per message (Message.max_segment_count, message.zig:310): more,
 * or a misaligned segment, gives INVALID_ARGUMENT (d_out_len 0, the slot untouched). Output
 * as in capnp_packed_encode_batch; d_out == NULL computes the packed sizes only. An empty
 * segment's address is checked for alignment and never read; with d_seg_count[i] == 0,
 * d_seg_first[i] is not used. Every d_status and d_out_len entry is written, whatever the
 * arrays held before the call. */
int capnp_packed_encode_message_batch(const uint64_t* d_seg_ptr, const uint64_t* d_seg_len,
                                      const uint32_t* d_seg_first, const uint32_t* d_seg_count, uint32_t n,
                                      uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                      uint64_t* d_out_len, int32_t* d_status, void* stream);

/* ------------------------------------------------------------------------
 * Encoder dialect: which packed bytes an encode call writes. An argument of the call (no
 * process-wide setting: it changes the bytes, and threads may use both at once).
 *   CAPNP_PACKED_DIALECT_ZIG  packPacked's bytes (message.zig:200-271): what every call
 *                             without a dialect argument writes. A literal run (tag FF) goes
 *                             on only over words without a zero byte.
 *   CAPNP_PACKED_DIALECT_CXX  the bytes of the C++ capnp packer (capnp convert binary:packed)
 *                             and pycapnp: a literal run opens at a word without a zero byte
 *                             and goes on over words with at most one zero byte; and packing
 *                             restarts at every piece the C++ message writer writes (a
 *                             message's segment table, then each segment), so no run crosses
 *                             from one piece to the next. A raw buffer is one piece. Never
 *                             larger than the Zig bytes; every decoder here reads both.
 * Any other value: INVALID_ARGUMENT, before any device work. With DIALECT_ZIG the calls
 * forward to capnp_packed_encode / _encode_batch_ws / _encoded_size_batch /
 * _encode_message_batch. Contracts (alignment, statuses, OUT_OF_SPACE, asynchrony, capture)
 * are those calls'. The C++ dialect runs one kernel, a wave per unit or message: it needs no
 * workspace (one passed is checked as the _ws calls check it, and not used) and never
 * allocates; units of at most 64 words have no lane-per-unit kernel yet.
 * ------------------------------------------------------------------------ */
#define CAPNP_PACKED_DIALECT_ZIG 0u /* message.zig:200-271, what every existing call emits */
#define CAPNP_PACKED_DIALECT_CXX 1u /* C++ capnp / pycapnp bytes */

/* capnp_packed_encode with a dialect. */
int capnp_packed_encode_dialect(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                                uint32_t dialect);

/* capnp_packed_encode_batch_ws with a dialect; d_out == NULL computes the packed sizes only
 * (capnp_packed_encoded_size_batch; d_out_off and d_out_cap may then be NULL). */
int capnp_packed_encode_batch_dialect(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                      uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                      const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                      uint32_t dialect, void* d_workspace, size_t workspace_bytes, void* stream);

/* capnp_packed_encode_message_batch with a dialect. Under DIALECT_CXX message i's bytes are the
 * packed segment table (8 * ceil((1 + count) / 2) bytes unpacked) followed by each packed
 * segment, every piece packed on its own. */
int capnp_packed_encode_message_batch_dialect(const uint64_t* d_seg_ptr, const uint64_t* d_seg_len,
                                              const uint32_t* d_seg_first, const uint32_t* d_seg_count, uint32_t n,
                                              uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                              uint64_t* d_out_len, int32_t* d_status, uint32_t dialect,
                                              void* stream);

/* ---------------------------------------------------------------------------
 * One dense packed stream: MessageBuilder.writePackedTo(writer) called for unit 0, 1, ...
 * n-1 on one writer (message.zig:2209-2213), in ONE pass over the input: no size pass, no
 * caller-side scan, no capacity slots.
 *   d_out_off[0] = out_base, d_out_off[i + 1] = d_out_off[i] + d_out_len[i]  (n + 1 entries);
 *   unit i's packed bytes are d_out[d_out_off[i] .. + d_out_len[i]), in unit order: the
 *   stream is the concatenation of packPacked(unit_i) (DIALECT_CXX: each unit one piece), byte
 *   for byte what encoded_size_batch -> lengths_to_offsets -> encode_batch writes.
 * out_base may be any byte value (odd ones append to a stream that already holds bytes);
 * d_out_off / d_out_len can be passed on unchanged as a decode's or
 * capnp_packed_read_message_batch's (in_off, in_len).
 * Per-unit input errors: a word side that is not 8-aligned INVALID_ARGUMENT, len % 8 != 0
 * INVALID_MESSAGE_SIZE, and a unit of more than 0xFFFFF000 words INVALID_ARGUMENT (this call
 * has no serial path for such units). Such a unit gets d_out_len 0, takes no bytes, and the
 * stream goes on.
 * Space: the stream may use d_out[0 .. out_cap). A unit with d_out_len > 0 whose end
 * d_out_off[i + 1] exceeds out_cap is not written and gets OUT_OF_SPACE; its d_out_len is
 * still its packed size and the offsets keep accumulating, so d_out_off[n] is the end a retry
 * needs. Units that end at or below out_cap are written and OK; a unit with nothing to write
 * is OK wherever it lands. No byte at or past d_out + out_cap and none below d_out + out_base
 * is ever written.
 * d_out == NULL: sizes and offsets only (out_cap is ignored): one call instead of
 * encoded_size_batch + lengths_to_offsets.
 * dialect: CAPNP_PACKED_DIALECT_ZIG or _CXX; anything else INVALID_ARGUMENT before any device
 * work.
 * d_workspace: caller-owned device memory, 256-B aligned, at least
 * capnp_packed_encode_dense_workspace_bytes(n) bytes, required for n > 0 (NULL, misaligned or
 * short: INVALID_ARGUMENT). The call zeroes it on `stream` every time; the library keeps no
 * state for this call and allocates nothing, so it is asynchronous and capturable in a
 * hipGraph. Two calls in flight must not share a workspace.
 * n == 0 is OK: d_out_off[0] = out_base when d_out_off is non-NULL, no device work when it is
 * NULL. The return value reports argument and launch errors only. A unit status of
 * DEVICE_ERROR means the kernel's bounded wait for an earlier unit's offset ran out (2 s of the
 * device's constant-rate clock; never expected. A single unit whose own encode takes longer
 * than that, on the order of a GiB, makes the units after it give up).
 * Units of at most 64 words take a wave each here, as in the C++ dialect.
 * ------------------------------------------------------------------------ */
size_t capnp_packed_encode_dense_workspace_bytes(uint32_t n);
int capnp_packed_encode_dense_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint8_t* d_out, uint64_t out_base, uint64_t out_cap,
                                    uint64_t* d_out_off /* n + 1 */, uint64_t* d_out_len /* n */,
                                    int32_t* d_status /* n */, uint32_t dialect, void* d_workspace,
                                    size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Framed messages as units: capnp_packed_encode_dialect,
 * capnp_packed_encode_batch_dialect and capnp_packed_encode_dense_batch with the framing known.
 * A unit is ONE framed message, the bytes toBytes writes (message.zig:2123-2170) and
 * Message.init parses (:341-394): the segment table (u32 count - 1, u32 words of each segment,
 * padded to a word), then the segments back to back. The framing is an argument of its own,
 * orthogonal to the dialect:
 *   DIALECT_CXX  the table (8 * ceil((1 + count) / 2) bytes) is packed as one piece, then every
 *                segment as a piece of its own: byte for byte what capnp convert binary:packed
 *                and pycapnp write for the message, and what
 *                capnp_packed_encode_message_batch_dialect writes from its segment list. (The
 *                unframed calls pack the whole unit as one piece, which differs for about half
 *                of all multi-segment messages and never for a single-segment one.)
 *   DIALECT_ZIG  packPacked(unit), exactly the unframed calls' bytes; the framing adds the checks.
 * Any other dialect: INVALID_ARGUMENT before any device work.
 * Per-unit checks, in this order; a failed unit gets d_out_len 0 and writes nothing (its slot
 * stays untouched; in the dense call it takes no bytes and the stream goes on):
 *   word side not 8-aligned          INVALID_ARGUMENT
 *   len % 8 != 0                     INVALID_MESSAGE_SIZE
 *   the table parse, as capnp_packed_message_init_batch: END_OF_STREAM (fewer than 4 bytes: an
 *     empty unit), INVALID_SEGMENT_COUNT, SEGMENT_COUNT_LIMIT_EXCEEDED (more than 512),
 *     TRUNCATED_MESSAGE (the table or a segment runs past the unit)
 *   words after the last segment     INVALID_ARGUMENT (Message.init ignores them; a stream
 *                                    writer must not: readPackedMessage would take them as the
 *                                    next message)
 *   more than 0xFFFFF000 words       INVALID_ARGUMENT
 * The table's padding half-word is packed as it stands, not checked. No load leaves the unit
 * beyond the aligned 16-byte lines it touches.
 * Every OK unit's output is exactly one packed message: capnp_packed_read_message_batch consumes
 * it whole (consumed == d_out_len, framed length == d_in_len).
 * Everything else is the mirrored call's contract: OUT_OF_SPACE reports the required size and
 * nothing is written at or past the capacity; d_out == NULL gives sizes only; the dense call
 * keeps the out_cap cut and the accumulating offsets (d_out_off has n + 1 entries). The batch
 * calls are asynchronous on `stream`, allocate nothing and keep no library state, so they are
 * capturable in a hipGraph. d_workspace is caller-owned device memory, 256-B aligned, required
 * for n > 0 (NULL, misaligned or short: INVALID_ARGUMENT): the slot call needs
 * capnp_packed_encode_framed_workspace_bytes(n) bytes, the dense call
 * capnp_packed_encode_dense_workspace_bytes(n). Two calls in flight must not share one.
 * n == 0 is OK with NULL arrays. capnp_packed_encode_framed is the host call for one message
 * (arguments as capnp_packed_encode_dialect).
 * ------------------------------------------------------------------------ */
int capnp_packed_encode_framed(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len,
                               uint32_t dialect);
size_t capnp_packed_encode_framed_workspace_bytes(uint32_t n);
int capnp_packed_encode_framed_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                     uint32_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                     const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                     uint32_t dialect, void* d_workspace, size_t workspace_bytes, void* stream);
int capnp_packed_encode_framed_dense_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                           uint32_t n, uint8_t* d_out, uint64_t out_base, uint64_t out_cap,
                                           uint64_t* d_out_off /* n + 1 */, uint64_t* d_out_len /* n */,
                                           int32_t* d_status /* n */, uint32_t dialect, void* d_workspace,
                                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Dense streams of packed messages split into their messages: what repeated
 * Reader.readPackedMessage calls on one reader consume (reader.zig:84-156), for n streams in
 * one call and without knowing where any message starts. Stream s is
 * d_in[d_in_off[s] .. + d_in_len[s]), at any byte alignment: a file written by
 * `capnp convert binary:packed`, a log of writePackedTo calls, or
 * capnp_packed_encode_dense_batch's stream without its offsets.
 * Per stream: the whole messages in order; d_consumed[s] = the packed bytes of those whole
 * messages (where the loop stopped); d_status[s] =
 *   OK                    every byte consumed (an empty stream: OK, 0 messages);
 *   END_OF_STREAM         the bytes end inside a message;
 *   INVALID_SEGMENT_COUNT, SEGMENT_COUNT_LIMIT_EXCEEDED, MESSAGE_TOO_LARGE,
 *   INVALID_PACKED_MESSAGE  the error of the message the loop stopped in; the messages before
 *                         it are still listed;
 *   INVALID_ARGUMENT      the stream has more than CAPNP_PACKED_SPLIT_MAX_STREAM_BYTES bytes: 0
 *                         messages, 0 consumed, none of its bytes read.
 * Message table: d_msg_first[s] = whole messages in the streams before s, d_msg_first[n] = the
 * total (n + 1 entries). Stream s owns rows [d_msg_first[s], d_msg_first[s + 1]) in stream
 * order; row k: d_msg_off[k] the message's first packed byte as an offset from d_in (not from
 * the stream), d_msg_len[k] its packed length, d_msg_framed[k] its framed length,
 * d_msg_stream[k] = s (d_msg_stream may be NULL). (d_msg_off, d_msg_len) pass unchanged as the
 * (in_off, in_len) of capnp_packed_decode_batch / capnp_packed_read_message_batch, and
 * capnp_packed_lengths_to_offsets(d_msg_framed) gives dense output offsets and exact
 * capacities.
 * Too few rows: d_msg_first always holds the full counts, so d_msg_first[n] is the max_msgs a
 * retry needs; rows k >= max_msgs are not written, nothing at or past index max_msgs of any
 * table is touched, statuses and d_consumed are unaffected, and the call still returns OK
 * (max_msgs 0: the tables may be NULL; counts, consumed and statuses only).
 * Reads: no result depends on a byte outside a stream's [off, off + len), and a message cut off
 * at a stream's end is never completed from the next stream's bytes. Loads are aligned 16-byte
 * chunks, as in every packed-side reader here: they may cover up to 15 bytes before a stream's
 * first and after its last byte, inside the 16-byte lines the stream itself touches.
 * Parallelism: across streams, and inside each 4608-byte window of a stream. From message to
 * message inside ONE stream the walk is serial: a message's start is only known from its
 * predecessor's header and end. One stream of very many small messages is therefore walked by
 * one wave, at about the cost of a window per message.
 * d_workspace: caller-owned device memory, 256-B aligned, at least
 * capnp_packed_split_workspace_bytes(n, 0) bytes, required for n > 0 (NULL, misaligned or
 * short: INVALID_ARGUMENT). in_bytes_bound is the caller's upper bound on the sum of d_in_len
 * (the lengths live on the device); it sizes the window tables that let a wave cross a window
 * its current message neither ends nor runs out of bytes in by one lookup. The tables are an
 * acceleration only: with a smaller workspace (down to in_bytes_bound 0), or past the table's
 * limit of n / 8 + 32768 windows, streams whose windows do not fit are walked window by window
 * and the results are the same. A kernel sets the workspace up on every call; the library
 * keeps no state for this call and allocates nothing, so it is asynchronous on `stream` and
 * capturable in a hipGraph. Two calls in flight must not share a workspace.
 * n == 0 writes d_msg_first[0] = 0 and nothing else (no workspace needed). The return value
 * reports argument and launch errors only.
 * ------------------------------------------------------------------------ */
#define CAPNP_PACKED_SPLIT_MAX_STREAM_BYTES (1ull << 40)
size_t capnp_packed_split_workspace_bytes(uint32_t n, uint64_t in_bytes_bound);
int capnp_packed_split_streams(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                               uint32_t n, uint64_t max_msgs, uint64_t* d_msg_first /* n + 1 */,
                               uint64_t* d_msg_off /* max_msgs */, uint64_t* d_msg_len /* max_msgs */,
                               uint64_t* d_msg_framed /* max_msgs */,
                               uint32_t* d_msg_stream /* max_msgs; may be NULL */, uint64_t* d_consumed /* n */,
                               int32_t* d_status /* n */, void* d_workspace, size_t workspace_bytes,
                               void* stream);

/* Message.init (message.zig:341-394) segment-table parse of n framed messages
 * d_in[d_in_off[i] .. + d_in_len[i]) (e.g. the output of a decode batch).
 * d_seg_count[i] = segments; segment j < max_segs of message i is
 * d_in[d_in_off[i] + d_seg_off[i*max_segs + j] .. + d_seg_len[i*max_segs + j]).
 * Errors per message: END_OF_STREAM (< 4 bytes), INVALID_SEGMENT_COUNT,
 * SEGMENT_COUNT_LIMIT_EXCEEDED, TRUNCATED_MESSAGE. Trailing bytes after the last
 * segment are ignored, as in the reference. d_in_off may be any byte value.
 * Rows: an OK message's entries j >= min(count, max_segs) are not written (segments past
 * max_segs are counted, not listed). A failed message gets d_seg_count 0; its row's content is
 * unspecified to this extent: entry j either is not written or holds segment j as the table
 * lists it (TRUNCATED_MESSAGE may list the segments before the one that runs past the data).
 * No message ever writes into another message's row. */
int capnp_packed_message_init_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint32_t n, uint32_t max_segs, uint32_t* d_seg_count, uint64_t* d_seg_off,
                                    uint64_t* d_seg_len, int32_t* d_status, void* stream);

/* Message.validate (message.zig:699-969, ValidationOptions :331-335) of n framed
 * messages d_in[d_in_off[i] .. + d_in_len[i]): Message.init's segment-table parse
 * (its errors: END_OF_STREAM, INVALID_SEGMENT_COUNT, SEGMENT_COUNT_LIMIT_EXCEEDED,
 * TRUNCATED_MESSAGE), then the depth-first pointer traversal with the reference's
 * limits and error order. d_status[i] = the first error the reference's recursion
 * would raise, or OK; d_words[i] (may be NULL) = traversal words consumed (OK only).
 * The reference defaults are segment_count_limit 512, traversal_limit_words 8 Mi,
 * nesting_limit 64. Any nesting_limit is accepted: up to 64 the call allocates nothing
 * and is capturable in a hipGraph; above 64, messages that need more than 64 stack frames
 * are validated by a second kernel with its frames in global memory, allocated
 * stream-ordered on `stream` (hipMallocAsync: 4n + 16 B and at most ~256 MiB of frame
 * stacks, freed stream-ordered). A nesting_limit above 2^18 is applied as 2^18 (far
 * deeper than the reference's recursive validate can go before its thread stack runs
 * out). A message of 4 GiB or more gets INVALID_ARGUMENT as its status. */
int capnp_packed_validate_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                uint32_t n, uint64_t segment_count_limit, uint64_t traversal_limit_words,
                                uint32_t nesting_limit, int32_t* d_status, uint64_t* d_words, void* stream);

/* ---------------------------------------------------------------------------
 * Reading fields of decoded messages on the device: getRootStruct
 * (message.zig:973-985), readStruct along a path (:1224-1235) and StructReader's scalar and
 * slice reads (:1051-1158, :1187-1198, :1259-1443) for n framed messages and n_fields fields
 * each, as columns. No schema: a field is a byte offset or a pointer index.
 *   kind        reference read                            offset        value / len / count
 *   U8..U64     readU8 / readU16 (readUnionDiscriminant)  byte offset   the value zero-extended / its
 *               / readU32 / readU64                       in the data   width in bytes / 1
 *   BOOL        readBool(offset, bit)                     section       0 or 1 / 1 / 1
 *   TEXT        readText                                  pointer       the content's byte offset FROM
 *   DATA        readData, readU8List (element size 2)     index         d_in / its byte length (bit
 *   LIST_BIT    readBoolList (1)                                        lists: (count + 7) / 8) / the
 *   LIST_16/32/64  readU16List / U32 and F32 / U64 and F64 (3, 4, 5)    element count
 * path: the struct the field is read from is root.readStruct(path[0])...readStruct(path[path_len - 1]).
 * `fields` is HOST memory and is passed to the kernel by value: no upload and no allocation, the
 * call is asynchronous on `stream`, keeps no library state and is capturable in a hipGraph.
 * Outputs are field-major: entry f * n + i is field f of message i, so d_value + f * n is a
 * column (d_count may be NULL). A failed entry gets value 0, len 0, count 0.
 * Message i is d_in[d_in_off[i] .. + d_in_len[i]) and starts at a multiple of 8; a misaligned
 * offset or a length of 4 GiB or more gives INVALID_ARGUMENT for every field of that message.
 * Per message, in the reference's order (the first error is the status of every field):
 *   Message.init's table parse, with capnp_packed_message_init_batch's statuses;
 *   getRootStruct: TRUNCATED_MESSAGE when segment 0 is shorter than 8 bytes (EMPTY_MESSAGE, no
 *     segments, cannot come out of the table parse: a table lists at least one);
 *   resolveStructPointer (:492-523) through resolvePointer with depth 8 (:451-490: single-far
 *     chains, the double-far landing pad and its content override): INVALID_SEGMENT_ID,
 *     OUT_OF_BOUNDS (a landing pad past its segment), INVALID_FAR_POINTER,
 *     NESTING_LIMIT_EXCEEDED (an eighth far hop), INVALID_POINTER (null, not a struct pointer, or
 *     a negative offset), TRUNCATED_MESSAGE (the struct runs past its segment).
 * Per field: each path step is readStruct: OUT_OF_BOUNDS (index past the pointer section),
 * INVALID_POINTER (null), then resolveStructPointer as above. Then
 *   data kinds: a field that does not lie wholly inside the data section
 *     (offset + width > 8 * data words) reads as the default: value 0, status OK, d_len 0,
 *     d_count 0 (the reference's schema-evolution rule);
 *   slice kinds (resolveListPointerAt, resolveListPointer :525-561): OUT_OF_BOUNDS (index past
 *     the section), INVALID_POINTER (null; not a list after resolution), resolvePointer's errors,
 *     OUT_OF_BOUNDS (a negative offset, or the content of the list AS ITS POINTER DESCRIBES IT
 *     runs past its segment), then INVALID_POINTER (the element size is not the kind's);
 *   TEXT (readText): an index past the section or a null pointer is OK with length 0; one
 *     trailing NUL byte is dropped from d_len and d_count.
 * Reference error names without a status of their own: InvalidRootPointer and InvalidTextPointer
 * are INVALID_POINTER, PointerDepthLimit is NESTING_LIMIT_EXCEEDED; InvalidSegmentId,
 * OutOfBounds, InvalidFarPointer, InvalidPointer, TruncatedMessage and EmptyMessage keep theirs.
 * Reads: every load is an aligned 8-byte word of the message's segment table or of one of its
 * segments (a 4-byte load when the message has fewer than 8 bytes); no byte outside
 * [off, off + len) is read.
 * Host-side checks, INVALID_ARGUMENT before any device work: n_fields > CAPNP_PACKED_MAX_FIELDS;
 * with n > 0 and n_fields > 0, a NULL array (d_count excepted), an unknown kind, bit > 7 or
 * bit != 0 on a kind other than BOOL, path_len > CAPNP_PACKED_MAX_PATH. n == 0 or n_fields == 0
 * is OK with no device work. Out of scope: capabilities, XOR defaults, the *Strict reads, UTF-8
 * validation; struct and pointer lists are capnp_packed_list_heads_batch's, below.
 * ------------------------------------------------------------------------ */
#define CAPNP_PACKED_FIELD_U8 0u       /* readU8 (message.zig:1120) */
#define CAPNP_PACKED_FIELD_U16 1u      /* readU16 (:1097), readUnionDiscriminant */
#define CAPNP_PACKED_FIELD_U32 2u      /* readU32 (:1074) */
#define CAPNP_PACKED_FIELD_U64 3u      /* readU64 (:1051) */
#define CAPNP_PACKED_FIELD_BOOL 4u     /* readBool (:1143) */
#define CAPNP_PACKED_FIELD_TEXT 5u     /* readText (:1417) */
#define CAPNP_PACKED_FIELD_DATA 6u     /* readData / readU8List (:1259, :1270): element size 2 */
#define CAPNP_PACKED_FIELD_LIST_BIT 7u /* readBoolList: element size 1 */
#define CAPNP_PACKED_FIELD_LIST_16 8u  /* readU16List: 3 */
#define CAPNP_PACKED_FIELD_LIST_32 9u  /* readU32List / F32: 4 */
#define CAPNP_PACKED_FIELD_LIST_64 10u /* readU64List / F64: 5 */
#define CAPNP_PACKED_MAX_FIELDS 32u
#define CAPNP_PACKED_MAX_PATH 4u
typedef struct capnp_packed_field {
    uint32_t kind;     /* CAPNP_PACKED_FIELD_* */
    uint32_t offset;   /* data kinds: byte offset in the data section; pointer kinds: pointer index */
    uint32_t bit;      /* BOOL: 0-7; otherwise 0 */
    uint32_t path_len; /* 0: the root struct; k: root.readStruct(path[0])...readStruct(path[k-1]) */
    uint32_t path[4];  /* pointer indices */
} capnp_packed_field;
int capnp_packed_read_fields_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                   uint32_t n, const capnp_packed_field* fields /* HOST */, uint32_t n_fields,
                                   uint64_t* d_value /* n_fields * n */, uint64_t* d_len /* n_fields * n */,
                                   uint64_t* d_count /* n_fields * n; may be NULL */,
                                   int32_t* d_status /* n_fields * n */, void* stream);

/* The slices as dense bytes: row i copies d_in[d_src_off[i] .. + d_src_len[i]) to
 * d_out[d_dst_off[i] ..), both sides at any byte alignment. A d_value / d_len column of
 * capnp_packed_read_fields_batch passes unchanged as (d_src_off, d_src_len), and
 * capnp_packed_lengths_to_offsets(d_len) gives dense destination offsets; offsets i * stride
 * into a zeroed buffer give a padded [n, stride] tensor.
 * A row that would end past out_cap (d_dst_off[i] + d_src_len[i] > out_cap, the sum taken
 * without wrapping) is not written and gets OUT_OF_SPACE; every other row is OK, and one of
 * length 0 touches nothing. Writes are byte-exact: no byte of d_out outside
 * a row's range is modified, so rows may be packed back to back. Loads are aligned 16-byte
 * chunks inside the 16-byte lines a row touches (the packed-side rule of every reader here).
 * Overlapping source and destination ranges are undefined. Asynchronous on `stream`, no
 * allocation, no library state, capturable in a hipGraph; n == 0 is OK with NULL arrays.
 * Parallelism: rows of at most 512 bytes are spread over a wave by 16-byte pieces; a longer row
 * is copied by ONE wave. A batch whose bytes sit in a handful of very long rows therefore runs
 * on a handful of waves; long rows are not tiled across waves. */
int capnp_packed_gather_batch(const uint8_t* d_in, const uint64_t* d_src_off, const uint64_t* d_src_len,
                              uint32_t n, uint8_t* d_out, const uint64_t* d_dst_off, uint64_t out_cap,
                              int32_t* d_status, void* stream);

/* ------------------------------------------------------------------------
 * Struct lists and pointer lists of decoded messages as element tables: the
 * "explode" of a columnar reader. Message i contributes count[i] elements, and a field of all
 * elements of all messages is one column of length sum(count). Three calls make the chain:
 *   capnp_packed_list_heads_batch      one list per message: where its elements lie, how many
 *   capnp_packed_lengths_to_offsets    d_count -> d_elem_start (n + 1 entries, base 0)
 *   capnp_packed_read_elements_batch   fields of every element, as columns over the elements
 * Both calls are asynchronous on `stream`, allocate nothing, keep no library state and are
 * capturable in a hipGraph; `path` and `fields` are HOST memory, passed to the kernels by value.
 *
 * capnp_packed_list_heads_batch resolves, per message, the list at pointer `pointer_index` of
 * the struct root.readStruct(path[0])...readStruct(path[path_len - 1]):
 *   CAPNP_PACKED_LIST_STRUCT   readStructList (message.zig:1165-1185), i.e.
 *                              resolveInlineCompositeList (:563-696)
 *   CAPNP_PACKED_LIST_POINTER  readTextList / readPointerList (:1200-1222): element size 6
 * d_count repeats head.count as a uint64 column of its own, so that it passes unchanged to
 * capnp_packed_lengths_to_offsets; d_status repeats head.status. A failed head is all zero but
 * for its status. Per message, in the reference's order (the first error is the status):
 *   the message-level checks of capnp_packed_read_fields_batch: a misaligned offset or a length
 *     of 4 GiB or more is INVALID_ARGUMENT; Message.init's table parse; getRootStruct; readStruct
 *     along `path`;
 *   the pointer slot: OUT_OF_BOUNDS (index past the pointer section), INVALID_POINTER (a null
 *     word: the reference returns an error for a null list pointer, not an empty list);
 *   LIST_STRUCT, resolveInlineCompositeList line by line (it does not go through resolvePointer:
 *   there is no depth-8 chain, and a far pointer that lands on a far pointer is an error):
 *     near list pointer: element size != 7 INVALID_INLINE_COMPOSITE_POINTER; a negative tag
 *       position OUT_OF_BOUNDS; the tag word past its segment OUT_OF_BOUNDS (readWord); tag type
 *       != 0, a negative count, or count * (data words + pointer words) > the pointer's word
 *       count INVALID_INLINE_COMPOSITE_POINTER; the pointer's word count * 8 past the segment
 *       OUT_OF_BOUNDS;
 *     single far: INVALID_SEGMENT_ID, OUT_OF_BOUNDS (the landing pad); a landing word that is not
 *       a list pointer INVALID_POINTER; then the near arm at the pad;
 *     double far: INVALID_SEGMENT_ID, OUT_OF_BOUNDS (the 16-byte pad); a first word that is not a
 *       single far pointer INVALID_FAR_POINTER; its segment INVALID_SEGMENT_ID; then by the second
 *       word: a struct-typed word is the tag (layout A: bounds on exactly count * words,
 *       OUT_OF_BOUNDS; :645's overflow guard, also OUT_OF_BOUNDS, cannot trip with 64-bit sizes);
 *       a list pointer (layout B: element size != 7 INVALID_INLINE_COMPOSITE_POINTER, the tag at
 *       the target checked as in the near arm); type 2 or 3 INVALID_INLINE_COMPOSITE_POINTER;
 *     pointer type 0 or 3: INVALID_POINTER;
 *   LIST_POINTER, resolveListPointerAt + resolveListPointer (:1187-1198, :525-561) exactly as the
 *     slice kinds of capnp_packed_read_fields_batch (resolvePointer's errors with depth 8, the
 *     bounds check on the list before the element size), then element size != 6 INVALID_POINTER.
 * Host-side checks, INVALID_ARGUMENT before any device work: an unknown list_kind; path_len >
 * CAPNP_PACKED_MAX_PATH; with n > 0 a NULL array (`path` may be NULL when path_len == 0).
 * n == 0 is OK with NULL arrays.
 *
 * capnp_packed_read_elements_batch. d_elem_start = lengths_to_offsets(d_count, base 0). Element
 * e lies in [0, min(d_elem_start[n], elem_cap)); it belongs to the message i with
 * d_elem_start[i] <= e < d_elem_start[i + 1] (empty lists own no element) and is element
 * k = e - d_elem_start[i] of that list: d_parent[e] = i, d_index[e] = k (either may be NULL).
 * Outputs are field-major over elem_cap: entry f * elem_cap + e is field f of element e. Entries
 * with e at or past the total are never written. The total stays on the device and the grid is
 * sized from elem_cap, so the call needs no sync. AN UNTRUSTED MESSAGE CAN CLAIM A VERY LARGE
 * LIST (a struct list of zero-word elements passes every check with up to 2^29 - 1 elements):
 * elem_cap is what bounds the work and the output.
 * If k >= d_head[i].count, the start array does not belong to these heads: every field of that
 * element is INVALID_ARGUMENT and nothing of the message is read.
 * The element is a struct reader:
 *   LIST_STRUCT: StructListReader.get (list_readers.zig:87-100): the struct at elems_off +
 *     k * 8 * (data_words + pointer_words) with the head's section sizes. get's own bounds check
 *     cannot fail after an OK head (the head's call checked the whole list against its segment),
 *     as EMPTY_MESSAGE cannot come out of a table parse.
 *   LIST_POINTER: the pointer slot elems_off + 8 k as a struct of no data words and one pointer.
 *     A descriptor with path_len 0, offset 0 and a slice kind is then check for check
 *     TextListReader.get / PointerListReader.getText (:113-133, :258-272: null is empty text with
 *     OK, element size != 2 INVALID_POINTER, one trailing NUL dropped), getData (:298-304) and
 *     get{U16,U32,U64,F32,F64,Bool}List (:252-256, :308-324: null INVALID_POINTER, bounds before
 *     the element size); one with path[0] == 0 is getStruct (:284-288) and then readStruct steps.
 * From the element onward a field means what it means in capnp_packed_read_fields_batch: path
 * steps, data reads with the schema-evolution default, slice reads, readText; `value` of a slice
 * is the content's byte offset from d_in, so columns feed capnp_packed_gather_batch unchanged.
 * The head's OK status stands for Message.init's checks, which are not redone: near pointers
 * read no table, a far pointer reads the segment count and the other segment's bounds from the
 * message's table. Reads: aligned 8-byte words of the message's table or of one of its segments,
 * no byte outside [off, off + len) of the element's own message.
 * Host-side checks, INVALID_ARGUMENT: those of capnp_packed_read_fields_batch on the descriptors;
 * elem_cap >= 2^32; an unknown list_kind; under LIST_POINTER a data kind with path_len 0, offset
 * != 0 with path_len 0, or path[0] != 0; with n > 0, elem_cap > 0 and n_fields > 0 a NULL array
 * (d_parent, d_index and d_count excepted). n_fields == 0 is legal with d_parent or d_index
 * non-NULL: the element numbering only. n == 0 or elem_cap == 0 is OK with no device work.
 * IndexOutOfBounds (get past the count) has no status and needs none: no element lies past it.
 * ------------------------------------------------------------------------ */
#define CAPNP_PACKED_LIST_STRUCT 0u  /* readStructList (message.zig:1165-1185): resolveInlineCompositeList */
#define CAPNP_PACKED_LIST_POINTER 1u /* readTextList / readPointerList (:1200-1222): element size 6 */
typedef struct capnp_packed_list_head { /* 32 bytes, device memory, one per message */
    uint64_t elems_off; /* byte offset FROM d_in of element 0 (struct list: first struct; pointer list: first pointer) */
    uint32_t count;     /* elements; 0 when status != OK */
    uint32_t segment;   /* the segment the elements lie in */
    uint32_t seg_begin; /* that segment's byte offset in the message */
    uint32_t seg_bytes; /* and its length */
    uint16_t data_words, pointer_words; /* struct list: from the tag; pointer list: 0, 1 */
    int32_t status;
} capnp_packed_list_head;
int capnp_packed_list_heads_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                  uint32_t n, const uint32_t* path /* HOST, path_len entries */,
                                  uint32_t path_len, uint32_t pointer_index, uint32_t list_kind,
                                  capnp_packed_list_head* d_head /* n */, uint64_t* d_count /* n */,
                                  int32_t* d_status /* n */, void* stream);
int capnp_packed_read_elements_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                     uint32_t n, const capnp_packed_list_head* d_head /* n */,
                                     const uint64_t* d_elem_start /* n + 1 */, uint32_t list_kind,
                                     uint64_t elem_cap, const capnp_packed_field* fields /* HOST */,
                                     uint32_t n_fields, uint32_t* d_parent /* elem_cap; may be NULL */,
                                     uint32_t* d_index /* elem_cap; may be NULL */, uint64_t* d_value,
                                     uint64_t* d_len, uint64_t* d_count /* may be NULL */,
                                     int32_t* d_status /* each n_fields * elem_cap */, void* stream);

/* ------------------------------------------------------------------------
 * Struct building over a batch: the inverse of capnp_packed_read_fields_batch
 * plus capnp_packed_gather_batch. One fixed sequence of builder calls (`ops`, HOST memory, passed
 * to the kernel by value as a plan) is applied to n messages whose values come from device
 * columns; message i leaves as the bytes of toBytes() at d_out + d_out_off[i]. The result feeds
 * capnp_packed_encode_framed_batch / _dense_batch unchanged.
 * Columns are op-major: entry k * n + i belongs to op k of message i.
 *   data kinds (U8..U64, BOOL)  the value is d_value's low bits; d_count is ignored, and so is
 *                               d_len unless it is CAPNP_PACKED_BUILD_ABSENT
 *   slice kinds                 the content is d_pool[d_value .. + d_len): TEXT without its NUL
 *                               (what the read returns), LIST_BIT with d_len the byte length and
 *                               d_count the element count, LIST_16/32/64 with d_len in bytes
 *   BUILD_STRUCT                ignores its column entries
 * so the (value, len, count) columns capnp_packed_read_fields_batch wrote pass back unchanged.
 * Per message the call runs this reference sequence, everything in segment 0, and takes
 * toBytes() (message.zig:2123-2170):
 *   MessageBuilder.init; allocateStruct(op0.data_words, op0.pointer_words) (:2061-2101);
 *   then each further op in order, an op whose d_len entry is CAPNP_PACKED_BUILD_ABSENT being
 *   skipped (BUILD_STRUCT ops always run), so that its pointer stays null / its bytes stay 0:
 *     U8..U64   writeU8/16/32/64(offset, value), non-strict: a write that does not lie wholly
 *               inside the target's data section is dropped (struct_builder.zig:356-430)
 *     BOOL      writeBool(offset, bit, value & 1) (:449-458)
 *     TEXT      writeText -> writeTextPointer (message.zig:1780-1815): len + 1 bytes with the NUL
 *     DATA, LIST_16/32/64, LIST_BIT   writeData / writeU16List .. / writeBoolList and a set of
 *               every element -> writeListPointer (:1909-1948): the pool bytes, padded to the word
 *               with zeros; bits past `count` in a bit list's last byte are written as 0
 *     BUILD_STRUCT  target.initStruct(offset, data_words, pointer_words) -> writeStructPointer
 *               (:1834-1886); (0, 0) writes a null pointer and allocates nothing
 * Every allocation is appended to segment 0 in op order. Later ops win where data writes overlap
 * (unions); BOOL is a read-modify-write of one bit.
 * Host-side checks, INVALID_ARGUMENT before any device work: n_ops > CAPNP_PACKED_MAX_BUILD_OPS;
 * with n > 0: n_ops == 0 or op 0 not BUILD_STRUCT, an unknown kind, bit > 7 or bit != 0 off BOOL,
 * non-zero reserved, target not an earlier BUILD_STRUCT op, a pointer index >= the target's
 * pointer_words (the reference's PointerIndexOutOfBounds, static here), two ops on one pointer
 * slot of one struct (the reference would orphan the first allocation), the words of every struct
 * + 1 > CAPNP_PACKED_MAX_BUILD_WORDS, a NULL array (d_pool may be NULL with pool_len 0; d_out NULL
 * asks for sizes only and then d_out_off / d_out_cap are not read), d_count NULL with a LIST_BIT
 * op. n == 0 is OK with NULL arrays.
 * Per message, the first that applies (a failed message writes no byte and gets d_out_len 0, but
 * OUT_OF_SPACE reports the needed length):
 *   1. d_out + d_out_off[i] is not a multiple of 8                          INVALID_ARGUMENT
 *   2. per slice op in order, not absent, and per op in this order:
 *        LIST_16/32/64 length not a multiple of the element width, or
 *        LIST_BIT with d_len != (d_count + 7) / 8                           INVALID_ARGUMENT
 *        an element count of 2^29 or more (TEXT: len + 1)                   LIST_TOO_LARGE
 *        the slice not inside [0, pool_len), the sum taken without wrapping OUT_OF_BOUNDS
 *   3. a framed length of 4 GiB or more                                     MESSAGE_TOO_LARGE
 *   4. the framed length > d_out_cap[i]                                     OUT_OF_SPACE
 * LIST_TOO_LARGE has no counterpart in the reference: its makeListPointer (message.zig:37-43)
 * silently drops the bits of a count that does not fit the pointer's 29, so no defined answer
 * exists for such a list. With d_out == NULL only d_out_len and d_status are produced and rules
 * 1 and 4 do not apply.
 * Contract: every byte of [d_out_off[i], + d_out_len[i]) of an OK message is written by the call
 * (the output need not be zeroed) and no byte of d_out outside those ranges is modified. Loads
 * from the pool are aligned 16-byte chunks that hold a byte of the slice (capnp_packed_gather_batch's
 * rule); nothing is read from the pool for a failed message. Asynchronous on `stream`, no
 * allocation, no workspace, no library state, no atomics, capturable in a hipGraph.
 * Parallelism: as capnp_packed_gather_batch. Slices of at most 512 bytes are spread over a wave
 * by 16-byte pieces; a longer slice is copied by ONE wave and is not tiled across waves.
 * Out of scope: other segments and the *InSegment variants, struct lists and pointer lists,
 * capabilities, the *Strict writes, rewriting a pointer.
 * ------------------------------------------------------------------------ */
#define CAPNP_PACKED_BUILD_STRUCT 16u        /* op 0: allocateStruct; later: StructBuilder.initStruct */
#define CAPNP_PACKED_BUILD_ABSENT UINT64_MAX /* a d_len entry: this op is not run for this message */
#define CAPNP_PACKED_MAX_BUILD_OPS 32u
#define CAPNP_PACKED_MAX_BUILD_WORDS 64u     /* the root pointer word + the words of every struct */
typedef struct capnp_packed_build_op {       /* 32 bytes, HOST memory, passed to the kernel by value */
    uint32_t kind;       /* CAPNP_PACKED_FIELD_U8 .. LIST_64 as a WRITE, or CAPNP_PACKED_BUILD_STRUCT */
    uint32_t target;     /* index of the BUILD_STRUCT op whose struct this op writes into
                            (for BUILD_STRUCT: the parent); ignored for op 0 */
    uint32_t offset;     /* data kinds: byte offset in target's data section;
                            slice kinds and BUILD_STRUCT: pointer index in target */
    uint32_t bit;        /* BOOL: 0-7; otherwise 0 */
    uint16_t data_words, pointer_words; /* BUILD_STRUCT only */
    uint32_t reserved[3]; /* 0 */
} capnp_packed_build_op;
int capnp_packed_build_fields_batch(const uint8_t* d_pool, uint64_t pool_len, uint32_t n,
                                    const capnp_packed_build_op* ops /* HOST */, uint32_t n_ops,
                                    const uint64_t* d_value /* n_ops * n */, const uint64_t* d_len /* n_ops * n */,
                                    const uint64_t* d_count /* n_ops * n; may be NULL when no op is LIST_BIT */,
                                    uint8_t* d_out /* NULL: sizes only */, const uint64_t* d_out_off,
                                    const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status,
                                    void* stream);

/* Exclusive scan of n lengths into n+1 offsets (d_off[0] = base, d_off[n] =
 * base + total), on device.
 * Turns capnp_packed_*_size_batch results into dense output offsets. The
 * caller supplies device scratch of capnp_packed_scan_scratch_bytes(n) bytes
 * (no allocation inside, so the call can be captured in a hipGraph). */
size_t capnp_packed_scan_scratch_bytes(uint32_t n);
int capnp_packed_lengths_to_offsets(const uint64_t* d_len, uint32_t n, uint64_t base,
                                    uint64_t* d_off, void* d_scratch, size_t scratch_bytes,
                                    void* stream);

/* Synthetic unit generator used by the benchmark and the parity tests:
 * n units of unit_bytes each, laid out densely from d_out (unit i at
 * i*unit_bytes). Byte k of word w of global unit u = unit_base + i is
 *   h  = mix64(seed, u, w); h2 = mix64(seed ^ 0xA5A5..., u, w)
 *   b  = ((h >> 8k) & 0xFF) < zero_thresh ? 0 : 1 + (((h2 >> 8k) & 0xFF) % 255)
 * i.e. zero with probability zero_thresh/256. */
int capnp_packed_generate(uint8_t* d_out, uint64_t n_units, uint64_t unit_bytes,
                          uint64_t unit_base, uint64_t seed, uint32_t zero_thresh,
                          void* stream);

/* Decoder selection for the batch decode of mid-size units (a tuning knob, not a
 * semantic one: every decoder is bit-exact):
 *   CAPNP_PACKED_DECODER_TWO_PASS  index pass + fill pass (the packed bytes are read twice);
 *   CAPNP_PACKED_DECODER_WORDS     single read: lane per unit, one output word per step
 *                                  (round 5; a failed unit may hold a prefix
 *                                  of its output unless capnp_packed_set_all_or_nothing(1));
 *   CAPNP_PACKED_DECODER_AUTO      the library's default: the words decoder for the mid units of
 *                                  more than 1280 packed bytes into slots of at most 8 KiB when a
 *                                  batch has at least a resident grid of them (~196K units on
 *                                  MI355X), the two-pass decoder for the rest;
 *                                  all two-pass under capnp_packed_set_all_or_nothing(1).
 * The words decoder steps one output word at a time and stops a unit at its slot's capacity
 * (its size then comes from a record walk), so no unit costs it more than out_cap / 8 steps.
 * Removed in round 5 (source at 869fccf), both measured slower than the
 * two-pass decoder: CAPNP_PACKED_DECODER_FUSED (per-lane 8-state entry maps) and
 * CAPNP_PACKED_DECODER_STREAM (lane-per-unit walk by 64-B windows); the library returns
 * CAPNP_PACKED_INVALID_ARGUMENT for them.
 * Returns the previous value; applies to batches enqueued after the call (process-wide). */
enum {
    CAPNP_PACKED_DECODER_AUTO = 0,
    CAPNP_PACKED_DECODER_TWO_PASS = 1,
    CAPNP_PACKED_DECODER_FUSED = 2,
    CAPNP_PACKED_DECODER_STREAM = 3,
    CAPNP_PACKED_DECODER_WORDS = 4
};
int capnp_packed_set_decoder(int decoder);

/* All-or-nothing for small decode units too (process-wide, for batches enqueued from
 * now on; returns the previous setting, 0 or 1). Long units, and mid units the two-pass
 * decoder takes, always leave a failed unit's slot untouched (message.zig:90 raises before any
 * output). Small units (<= 512 packed bytes into <= 8-KiB slots) are by default decoded a lane
 * each in one streaming pass, and mid units the words decoder takes (see
 * capnp_packed_set_decoder) stream their output out as they go: a failed one may keep a prefix
 * of its output (never a byte past out_cap), at any batch size (the default contract above). With on != 0, small units are decoded through LDS
 * and stored only when OK, and every mid unit goes to the two-pass decoder, at a cost (C5
 * decode 0.69 -> 0.79 ms; the headline decode 2.0 -> 2.5 ms). */
int capnp_packed_set_all_or_nothing(int on);

/* Launch policy (process-wide, for batches enqueued from now on; returns the previous flags;
 * unknown bits are ignored). No result depends on it, only where the kernels run:
 *   CAPNP_PACKED_LAUNCH_LONG_INLINE      long units run after the main grid on the caller's stream
 *                                        instead of on a side stream forked from and joined into it;
 *   CAPNP_PACKED_LAUNCH_MID_SIDE_STREAM  encode and decode: mid units on a second side stream beside
 *                                        the small units' kernel (helps batches of mostly small units
 *                                        with a few mid ones; costs a fork/join
 *                                        otherwise);
 *   CAPNP_PACKED_LAUNCH_CLASS_SCAN       the class pass's scan as a kernel of its own also for
 *                                        batches of at most 1M units (by default their scatter
 *                                        kernel does it; larger batches always launch it). */
#define CAPNP_PACKED_LAUNCH_LONG_INLINE 0x1u
#define CAPNP_PACKED_LAUNCH_MID_SIDE_STREAM 0x2u
#define CAPNP_PACKED_LAUNCH_CLASS_SCAN 0x4u
uint32_t capnp_packed_set_launch_flags(uint32_t flags);

#ifdef __cplusplus
}
#endif

#endif /* CAPNP_PACKED_H */
