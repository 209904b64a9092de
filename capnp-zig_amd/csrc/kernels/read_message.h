// kernels/read_message.h
// Reader.readPackedMessage, batched, pass 1: the packed header's parse (packed_header: the
// status and the framed length of the message at the front of a packed stream; the framer and
// the splitter parse every message's header with it) and read_header_kernel, which routes each
// message to the words decoder or to the walk / gate passes. The later passes are the decoders'
// (decode_words_kernel<true>, decode_index_kernel's kRdWalk / kRdGate, decode_wave_kernel;
// launch_read_message). DESIGN.md §2.4.
// Leans on:
//   common.h             kBlock, kRdWordsMax, kStWords, kStNeedWalk, the ST_* statuses
//   device_helpers.h     ld_u64
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"

namespace cpk {

// ---------------------------------------------------------------------------
// Reader.readPackedMessage, batched (reader.zig:84-156)
// ---------------------------------------------------------------------------
// Unit i is one reader's buffered packed stream; one message is decoded from its
// front (launch_read_message):
//   1. read_header_kernel: lane per unit, decodes records until the segment table
//      is complete (one record for a 1-segment message) and writes the framed
//      length to out_len, or the header error to status;
//      (ROUTE: messages of at most kRdWordsMax framed words kStWords, longer ones kStNeedWalk);
//   2. messages of more than kRdWordsMax words: decode_index_kernel<true, kRdWalk> (the walk
//      alone, consumed) and decode_index_kernel<false, kRdGate> (the records over in_len =
//      consumed), then the fill pass and the full-path fallback over in_len = consumed;
//   3. the others: decode_words_kernel<true> (round 6), which stops each lane's walk at the
//      first record boundary that reaches the framed length and applies the reader's
//      overshoot / end-of-stream rules there; consumed = the bytes it walked.
constexpr uint64_t kMaxTotalWords = 8ull * 1024 * 1024;  // reader.zig:6
constexpr uint64_t kMaxSegments = 512;                   // message.zig:310
constexpr uint64_t kHdrMaxWords = 257;                   // (1 + 512 + pad) u32 = 257 words

// Pass 1. Checks follow the reference's order: a record cut short by the end of
// the stream (EndOfStream), then after the first record InvalidSegmentCount /
// SegmentCountLimitExceeded (reader.zig:121-125), then once header_bytes are
// decoded MessageTooLarge (:140). Segment sizes are summed from the header's
// words as the records produce them (zero words add nothing). packed_header returns the
// status and, when OK, the framed length in `needed`.
__device__ int32_t packed_header(const uint8_t* __restrict__ p, uint64_t P, uint64_t& needed) {
    uint64_t r = 0;          // read cursor
    uint64_t words = 0;      // decoded words (out.items.len / 8)
    uint64_t count = 0;      // segment count (set by word 0)
    uint32_t count_m1 = 0;
    uint64_t total = 0;      // sum of the sizes decoded so far
    needed = 0;
    for (;;) {
        if (r >= P) return ST_EOS;  // :95 readByte
        const uint32_t t = p[r++];
        uint64_t w0 = 0;
        uint32_t c = 0;
        const uint8_t* lit = p;
        if (t == 0x00) {  // :96-99
            if (r >= P) return ST_EOS;
            c = p[r++];
        } else if (t == 0xFF) {  // :100-110
            if (P - r < 9) return ST_EOS;
            w0 = ld_u64(p + r);
            c = p[r + 8];
            r += 9;
            if (P - r < 8ull * c) return ST_EOS;
            lit = p + r;
            r += 8ull * c;
        } else {  // :111-119
            if (P - r < (uint64_t)__popc(t)) return ST_EOS;
            for (uint32_t k = 0; k < 8; ++k)
                if ((t >> k) & 1u) w0 |= (uint64_t)p[r++] << (8 * k);
        }
        // the record's words that hold header u32s: u32 j of the frame is
        // segment count - 1 (j = 0) or the size of segment j - 1 (1 <= j <= count)
        const uint64_t nw = 1ull + c;
        if (words == 0) {
            count_m1 = (uint32_t)w0;
            count = (uint64_t)count_m1 + 1;
        }
        if (t != 0x00) {
            for (uint64_t i = 0; i < nw && words + i < kHdrMaxWords; ++i) {
                const uint64_t w = i == 0 ? w0 : ld_u64(lit + 8 * (i - 1));
                const uint64_t j = 2 * (words + i);
                if (j >= 1 && j <= count) total += (uint32_t)w;
                if (j + 1 <= count) total += w >> 32;
            }
        }
        words += nw;
        // :121-144 (out.items.len >= 4 after any record)
        if (count_m1 == 0xFFFFFFFFu) return ST_SEGCOUNT;
        if (count > kMaxSegments) return ST_SEGLIMIT;
        const uint64_t header_bytes = 4 * (1 + count + ((count & 1) ? 0 : 1));
        if (8 * words >= header_bytes) {
            if (total > kMaxTotalWords) return ST_TOOLARGE;
            needed = header_bytes + 8 * total;
            return ST_OK;
        }
    }
}

// ROUTE (launch_read_message): a message of at most kRdWordsMax framed words goes to the words
// decoder (kStWords), a longer one to the walk passes (kStNeedWalk); errors stand.
template <bool ROUTE>
__global__ __launch_bounds__(kBlock) void read_header_kernel(const uint8_t* __restrict__ in,
                                                             const uint64_t* __restrict__ in_off,
                                                             const uint64_t* __restrict__ in_len, uint32_t n,
                                                             uint64_t* __restrict__ out_len,
                                                             uint64_t* __restrict__ consumed,
                                                             int32_t* __restrict__ status) {
    const uint32_t unit = blockIdx.x * kBlock + threadIdx.x;
    if (unit >= n) return;
    uint64_t needed = 0;
    const int32_t st = packed_header(in + in_off[unit], in_len[unit], needed);
    status[unit] = (ROUTE && st == ST_OK) ? ((needed >> 3) <= kRdWordsMax ? kStWords : kStNeedWalk) : st;
    out_len[unit] = st == ST_OK ? needed : 0;
    consumed[unit] = 0;
}

}  // namespace cpk
