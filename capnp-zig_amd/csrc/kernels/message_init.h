// kernels/message_init.h
// Message.init on device: message_init_kernel, the segment table of each framed message, lane
// per message. DESIGN.md §2.5.
// Leans on:
//   common.h             kBlock, kMsgMaxSegs, the ST_* statuses
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"

namespace cpk {

// ---------------------------------------------------------------------------
// Message.init on device (message.zig:341-394): the segment table of each framed
// message, lane per message. seg_off / seg_len get max_segs entries per message
// (row i at i * max_segs; segments past max_segs are counted, not listed).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void message_init_kernel(const uint8_t* __restrict__ in,
                                                              const uint64_t* __restrict__ in_off,
                                                              const uint64_t* __restrict__ in_len, uint32_t n,
                                                              uint32_t max_segs, uint32_t* __restrict__ seg_count,
                                                              uint64_t* __restrict__ seg_off,
                                                              uint64_t* __restrict__ seg_len,
                                                              int32_t* __restrict__ status) {
    const uint32_t msg = blockIdx.x * kBlock + threadIdx.x;
    if (msg >= n) return;
    const uint8_t* const d = in + in_off[msg];
    const uint64_t len = in_len[msg];
    auto u32at = [&](uint64_t o) {
        return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24);
    };
    int32_t st = ST_OK;
    uint64_t count = 0;
    if (len < 4) {
        st = ST_EOS;  // :343 readInt
    } else {
        const uint32_t m1 = u32at(0);
        if (m1 == 0xFFFFFFFFu) st = ST_SEGCOUNT;  // :346
        else if ((uint64_t)m1 + 1 > kMsgMaxSegs) st = ST_SEGLIMIT;  // :348
        else {
            count = (uint64_t)m1 + 1;
            const uint64_t header = 4 * (1 + count + ((count & 1) ? 0 : 1));
            if (header > len) st = ST_TRUNC;  // :353
            uint64_t o = header;
            for (uint64_t i = 0; st == ST_OK && i < count; ++i) {
                const uint64_t end = o + 8ull * u32at(4 + 4 * i);
                if (end > len) { st = ST_TRUNC; break; }  // :380
                if (i < max_segs) {
                    seg_off[(uint64_t)msg * max_segs + i] = o;
                    seg_len[(uint64_t)msg * max_segs + i] = end - o;
                }
                o = end;
            }
        }
    }
    seg_count[msg] = st == ST_OK ? (uint32_t)count : 0u;
    status[msg] = st;
}

}  // namespace cpk
