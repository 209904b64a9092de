// kernels/common.h
// Wave / block constants, the ST_* statuses (capnp_packed.h's codes) and the internal kSt*
// statuses that one pass leaves for the next, and the few limits that more than one path checks
// (so that no path includes another for a constant). Included by every header under kernels/ that
// names a status or a block size.
// DESIGN.md §2 (execution model), §2.4 (the read-message statuses).
#pragma once
#include <stdint.h>

#include "capnp_packed.h"

namespace cpk {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;

// ---- encode fast path ------------------------------------------------------
constexpr uint32_t kEncMaxWords = 512;                 // 4 KiB unpacked unit
constexpr uint32_t kEncRow = 80;                       // 64 B words + 16 B pad per lane row
constexpr uint32_t kEncLds = 64 * kEncRow;             // 5120 B; reused for the packed output
// max packed size of 512 words is 9*512+1 = 4609 B; + 16 B align slack + 16 B round-up <= 5120

enum : int32_t {
    ST_OK = CAPNP_PACKED_OK,
    ST_SIZE = CAPNP_PACKED_INVALID_MESSAGE_SIZE,
    ST_EOF = CAPNP_PACKED_UNEXPECTED_EOF,
    ST_SPACE = CAPNP_PACKED_OUT_OF_SPACE,
    ST_ARG = CAPNP_PACKED_INVALID_ARGUMENT,
    ST_DEVERR = CAPNP_PACKED_DEVICE_ERROR,  // a kernel's own loop guard tripped (never expected)
    // Reader.readPackedMessage (reader.zig:84-156)
    ST_EOS = CAPNP_PACKED_END_OF_STREAM,
    ST_SEGCOUNT = CAPNP_PACKED_INVALID_SEGMENT_COUNT,
    ST_SEGLIMIT = CAPNP_PACKED_SEGMENT_COUNT_LIMIT_EXCEEDED,
    ST_TOOLARGE = CAPNP_PACKED_MESSAGE_TOO_LARGE,
    ST_OVERSHOOT = CAPNP_PACKED_INVALID_PACKED_MESSAGE,
    ST_TRUNC = CAPNP_PACKED_TRUNCATED_MESSAGE,  // Message.init (message.zig:353/380)
    // Message.validate (message.zig:699-969)
    ST_EMPTY = CAPNP_PACKED_EMPTY_MESSAGE,
    ST_NEST = CAPNP_PACKED_NESTING_LIMIT_EXCEEDED,
    ST_SEGID = CAPNP_PACKED_INVALID_SEGMENT_ID,
    ST_PTR = CAPNP_PACKED_INVALID_POINTER,
    ST_OOB = CAPNP_PACKED_OUT_OF_BOUNDS,
    ST_TRAV = CAPNP_PACKED_TRAVERSAL_LIMIT_EXCEEDED,
    ST_FAR = CAPNP_PACKED_INVALID_FAR_POINTER,
    ST_ICP = CAPNP_PACKED_INVALID_INLINE_COMPOSITE_POINTER,
    ST_LIST = CAPNP_PACKED_LIST_TOO_LARGE,
};
// internal status between decode passes: the unit goes to a full (fallback) decoder
constexpr int32_t kStNeedFull = 0x7FFF0001;
constexpr int32_t kStNeedWalk = 0x7FFF0002;  // read-message: the one-pass walk could not take the unit
constexpr int32_t kStNeedGate = 0x7FFF0003;  // read-message: walked (consumed known), records next
constexpr int32_t kStWords = 0x7FFF0005;     // read-message: the words decoder's (read_header_kernel)
constexpr uint64_t kRdWordsMax = 1024;       // read-message: framed words the words decoder takes
// status of a long unit between its listing and its worker's result
constexpr int32_t kStPending = CAPNP_PACKED_DEVICE_ERROR;

// ---- limits more than one path checks --------------------------------------
// the encoders of segment lists, Message.init and Message.validate
constexpr uint32_t kMsgMaxSegs = 512;  // Message.max_segment_count (message.zig:310)
// the class pass (unit_class) and the small-unit decoders
constexpr uint64_t kSmDecP = 512;     // decode: small = at most 512 packed bytes ...
constexpr uint64_t kSmDecCap = 8192;  // ... into a slot of at most 8 KiB
// the index walk and the words decoder
constexpr uint64_t kIxSizeMax = 1ull << 31;       // size-only walk: longer units use decode_size_lane_kernel
// the tile table (encode), the window table (decode, framer) and the splitter's message table
constexpr uint32_t kTileSkip = 0xFFFFFFFFu;  // a table entry of a unit that went to the serial list

}  // namespace cpk
