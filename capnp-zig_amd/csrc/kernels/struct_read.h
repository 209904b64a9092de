// kernels/struct_read.h
// Reads on decoded messages: read_fields_kernel (getRootStruct, readStruct along a path, the
// scalar and slice reads of StructReader as columns, lane per message) and gather_kernel (the
// slices as dense bytes, a ragged byte copy). DESIGN.md §2.13.
// Leans on:
//   common.h             kWave, kBlock, the ST_* statuses
//   device_helpers.h     lane_id, readlane, shfl_u64, wave_incl_sum, wave_lds_sync, store_partial16
//   message_walk.h       mw_init, MwSegsLds, mw_root, mw_read_fields, MwStage, SrFields, kSrSegs, kSrGroup
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"
#include "kernels/message_walk.h"

namespace cpk {

// ---------------------------------------------------------------------------
// read_fields_kernel: Message.init, getRootStruct (message.zig:973-985), then every field of the
// descriptor table in turn from the root struct, lane per message; the results go out through
// LDS a group of fields at a time (message_walk.h has each of these and says why).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void read_fields_kernel(const uint8_t* __restrict__ in,
                                                             const uint64_t* __restrict__ in_off,
                                                             const uint64_t* __restrict__ in_len, uint32_t n,
                                                             const SrFields fs, uint32_t n_fields,
                                                             uint64_t* __restrict__ value,
                                                             uint64_t* __restrict__ flen,
                                                             uint64_t* __restrict__ count,
                                                             int32_t* __restrict__ status) {
    __shared__ uint32_t segb_all[(kSrSegs + 1) * kBlock];  // bound i of thread t at [i * kBlock + t]
    __shared__ uint32_t res_all[4 * kSrGroup * kBlock];    // dword i of thread t's field g at [(4 g + i) * kBlock + t]
    const uint32_t msg = blockIdx.x * kBlock + threadIdx.x;
    if (msg >= n) return;
    const uint64_t moff = in_off[msg];
    const uint64_t len = in_len[msg];
    const uint8_t* const d = in + moff;
    const MwStage out{res_all + threadIdx.x, msg, n, value, flen, count, status};
    auto fail_all = [&](int32_t st) { out.store_all(n_fields, st); };

    uint32_t nseg;
    if (int32_t st = mw_init(d, moff, len, segb_all + threadIdx.x, nseg)) return fail_all(st);
    MwSegsLds sg{d, nseg, segb_all + threadIdx.x};
    MwStruct root{};
    if (int32_t st = mw_root(sg, root)) return fail_all(st);
    mw_read_fields(sg, moff, root, fs, n_fields, out);
}

// ---------------------------------------------------------------------------
// gather_kernel: row i = in[src_off[i] .. + src_len[i]) to out[dst_off[i] ..), any byte
// alignment on both sides. A row is cut into the aligned 16-byte chunks of its DESTINATION
// (pieces); a piece's bytes come from the one or two aligned 16-byte source chunks that hold
// them (only chunks that hold a byte of the row are loaded), and a piece that is not a whole
// chunk is stored byte-exact (store_partial16), so neighbouring rows may share chunks.
// A wave takes 64 rows: the pieces of its rows of at most kGaShort bytes are flattened over
// the lanes (a prefix sum of piece counts, the owner of a piece found by bisection); each
// longer row then takes the whole wave, 64 pieces a turn.
// ---------------------------------------------------------------------------
constexpr uint32_t kGaShort = 512;  // rows up to this many bytes are flattened across the wave

// piece p of a row: src and dst are ADDRESSES (the chunks are aligned in memory, not in the
// caller's offsets)
__device__ __forceinline__ void gather_piece(uint64_t src, uint64_t dst, uint64_t len, uint64_t p) {
    const uint64_t c16 = (dst & ~15ull) + 16 * p;
    const uint32_t lo = p == 0 ? (uint32_t)(dst & 15) : 0u;
    const uint64_t end = dst + len;
    const uint32_t hi = end - c16 < 16 ? (uint32_t)(end - c16) : 16u;
    // chunk byte b is source byte t + b, for b in [lo, hi)
    const uint64_t t = src + (c16 - dst);  // wraps below src for b < lo: only bytes >= lo are used
    const uint64_t a = t & ~15ull;
    const uint32_t sh = (uint32_t)(t & 15);
    uint4 A = make_uint4(0, 0, 0, 0), B = A;
    if (sh + lo < 16) A = *reinterpret_cast<const uint4*>(a);
    if (sh + hi > 16) B = *reinterpret_cast<const uint4*>(a + 16);
    // 32 bytes A:B shifted down by sh bytes
    const uint64_t q0 = (uint64_t)A.x | ((uint64_t)A.y << 32), q1 = (uint64_t)A.z | ((uint64_t)A.w << 32);
    const uint64_t q2 = (uint64_t)B.x | ((uint64_t)B.y << 32), q3 = (uint64_t)B.z | ((uint64_t)B.w << 32);
    const uint64_t u0 = sh & 8 ? q1 : q0, u1 = sh & 8 ? q2 : q1, u2 = sh & 8 ? q3 : q2;
    const uint32_t s = (sh & 7) * 8;
    const uint64_t x0 = s ? (u0 >> s) | (u1 << (64 - s)) : u0;
    const uint64_t x1 = s ? (u1 >> s) | (u2 << (64 - s)) : u1;
    if (lo == 0 && hi == 16)
        *reinterpret_cast<uint4*>(c16) =
            make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
    else
        store_partial16(reinterpret_cast<uint8_t*>(c16), lo, hi, x0, x1);
}

// pieces of a row: the destination's aligned 16-byte chunks it touches
__device__ __forceinline__ uint64_t gather_pieces(uint64_t dst, uint64_t len) {
    return len ? ((dst + len + 15) >> 4) - (dst >> 4) : 0;
}

__global__ __launch_bounds__(kBlock) void gather_kernel(const uint8_t* __restrict__ in,
                                                        const uint64_t* __restrict__ src_off,
                                                        const uint64_t* __restrict__ src_len, uint32_t n,
                                                        uint8_t* __restrict__ out,
                                                        const uint64_t* __restrict__ dst_off, uint64_t out_cap,
                                                        int32_t* __restrict__ status) {
    __shared__ uint64_t s_src[kBlock], s_dst[kBlock];
    __shared__ uint32_t s_len[kBlock], s_pfx[kBlock];
    const uint32_t lane = lane_id();
    const uint32_t wbase = threadIdx.x - lane;  // this wave's slice of the arrays
    const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
    uint64_t src = 0, dst = 0, len = 0;
    if (row < n) {
        src = src_off[row];
        dst = dst_off[row];
        len = src_len[row];
        int32_t st = ST_OK;
        if (len > out_cap || dst > out_cap - len) {  // would end past out_cap: not written
            st = ST_SPACE;
            len = 0;
        }
        status[row] = st;
    }
    src += reinterpret_cast<uint64_t>(in);  // addresses from here on
    dst += reinterpret_cast<uint64_t>(out);
    // ---- short rows, flattened ---------------------------------------------------------------
    const bool is_short = len <= kGaShort;
    const uint32_t np = is_short ? (uint32_t)gather_pieces(dst, len) : 0u;
    const uint32_t incl = wave_incl_sum(np);
    const uint32_t total = readlane(incl, kWave - 1);
    s_src[threadIdx.x] = src;
    s_dst[threadIdx.x] = dst;
    s_len[threadIdx.x] = is_short ? (uint32_t)len : 0u;
    s_pfx[threadIdx.x] = incl;
    wave_lds_sync();
    for (uint32_t j = lane; j < total; j += kWave) {
        // the first row k with pfx[k] > j
        uint32_t k = 0;
#pragma unroll
        for (uint32_t step = kWave / 2; step; step >>= 1)
            if (s_pfx[wbase + k + step - 1] <= j) k += step;
        const uint32_t before = k ? s_pfx[wbase + k - 1] : 0u;
        gather_piece(s_src[wbase + k], s_dst[wbase + k], s_len[wbase + k], j - before);
    }
    // ---- long rows, a wave each ---------------------------------------------------------------
    uint64_t longs = __ballot(!is_short);
    while (longs) {
        const uint32_t k = (uint32_t)__builtin_ctzll(longs);
        longs &= longs - 1;
        const uint64_t rs = shfl_u64(src, k), rd = shfl_u64(dst, k), rl = shfl_u64(len, k);
        const uint64_t pieces = gather_pieces(rd, rl);
        for (uint64_t p = lane; p < pieces; p += kWave) gather_piece(rs, rd, rl, p);
    }
}

}  // namespace cpk
