// kernels/decode_size_lane.h
// The size pass's fallback: decode_size_lane_kernel, the decoded size of the units the size-only
// index walk declines (kIxSizeMax packed bytes or more), lane per unit over a register window
// (view_byte, load_piece). DESIGN.md §2.3.
// Leans on:
//   common.h             kBlock, kStNeedFull, the ST_* statuses
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"

namespace cpk {

// ---------------------------------------------------------------------------
// Decoded size, lane per unit: the size pass's fallback for units of kIxSizeMax (2 GiB) packed
// bytes or more, which the size-only index walk declines (kStNeedFull; launch_decode)
// ---------------------------------------------------------------------------
// Each lane owns ONE unit and walks its record chain (tag -> record length) exactly once,
// counting the words. The lane keeps a sliding window of its packed bytes in registers: a
// 32-byte view (q0..q3) plus one 16-byte piece in flight (n0, n1).

// View helper takes the window by value so the selects stay register selects
// (members selected through `this` were turned into an indexed alloca in LDS).
__device__ __forceinline__ uint32_t view_byte(uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, uint32_t o) {
    uint64_t a = (o & 8) ? q1 : q0;  // o < 32
    uint64_t b = (o & 8) ? q3 : q2;
    uint64_t q = (o & 16) ? b : a;
    return (uint32_t)(q >> (8 * (o & 7))) & 0xFFu;
}
__device__ __forceinline__ void load_piece(const uint8_t* base, uint32_t npieces, uint32_t idx, uint64_t& a,
                                           uint64_t& b) {
    if (idx < npieces) {
        uint4 v = *reinterpret_cast<const uint4*>(base + 16 * (uint64_t)idx);
        a = (uint64_t)v.x | ((uint64_t)v.y << 32);
        b = (uint64_t)v.z | ((uint64_t)v.w << 32);
    } else {
        a = 0;
        b = 0;
    }
}

// out / out_off / out_cap are not read (the launcher passes the batch's arguments as they are).
__global__ __launch_bounds__(kBlock) void decode_size_lane_kernel(const uint8_t* __restrict__ in,
                                                                  const uint64_t* __restrict__ in_off,
                                                                  const uint64_t* __restrict__ in_len,
                                                                  uint32_t n, uint8_t* __restrict__ out,
                                                                  const uint64_t* __restrict__ out_off,
                                                                  const uint64_t* __restrict__ out_cap,
                                                                  uint64_t* __restrict__ out_len,
                                                                  int32_t* __restrict__ status) {
    const uint32_t unit = blockIdx.x * kBlock + threadIdx.x;
    if (unit >= n) return;
    if (status[unit] != kStNeedFull) return;  // only the units decode_index_kernel<true> declined
    const uint8_t* src = in + in_off[unit];
    const uint64_t P = in_len[unit];
    const uint32_t s = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15);
    const uint64_t end64 = s + P;
    const uint8_t* base = src - s;
    const uint32_t npieces = (uint32_t)((end64 + 15) >> 4);
    // window: q0..q3 = pieces wb/16, wb/16+1; n0,n1 = piece wb/16+2 (in flight)
    uint64_t q0, q1, q2, q3, n0, n1;
    uint32_t wb = 0;
    load_piece(base, npieces, 0, q0, q1);
    load_piece(base, npieces, 1, q2, q3);
    load_piece(base, npieces, 2, n0, n1);
    auto ensure = [&](uint32_t p) {
        while (p - wb >= 16) {
            q0 = q2; q1 = q3; q2 = n0; q3 = n1;
            wb += 16;
            load_piece(base, npieces, (wb >> 4) + 2, n0, n1);
        }
    };
    uint64_t pos = s;
    uint64_t wo = 0;
    int32_t st = ST_OK;
    while (pos < end64) {
        ensure((uint32_t)pos);
        const uint32_t o = (uint32_t)pos - wb;
        const uint32_t t = view_byte(q0, q1, q2, q3, o);
        if (t == 0x00) {  // message.zig:101-110
            if (pos + 2 > end64) { st = ST_EOF; break; }
            const uint32_t c = view_byte(q0, q1, q2, q3, o + 1);
            for (uint32_t k = 0; k <= c; ++k) ++wo;
            pos += 2;
        } else if (t == 0xFF) {  // message.zig:112-128
            if (pos + 10 > end64) { st = ST_EOF; break; }
            const uint32_t c = view_byte(q0, q1, q2, q3, o + 9);
            if (pos + 10 + 8ULL * c > end64) { st = ST_EOF; break; }
            ++wo;
            pos += 10;
            for (uint32_t k = 0; k < c; ++k) {  // the window follows the run (as the decoders read it)
                ensure((uint32_t)pos);
                ++wo;
                pos += 8;
            }
        } else {  // message.zig:131-141
            const uint32_t k = __popc(t);
            if (pos + 1 + k > end64) { st = ST_EOF; break; }
            ++wo;
            pos += 1 + k;
        }
    }
    if (st != ST_OK) {
        out_len[unit] = 0;
        status[unit] = st;
        return;
    }
    const uint64_t U = 8 * wo;
    out_len[unit] = U;
    status[unit] = ST_OK;
}

}  // namespace cpk
