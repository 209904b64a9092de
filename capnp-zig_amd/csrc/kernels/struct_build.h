// kernels/struct_build.h
// The write side of struct_read.h: build_fields_kernel builds one single-segment framed message
// per row from columns (MessageBuilder.allocateStruct, the StructBuilder writes and toBytes,
// message.zig:1643-2170, message/struct_builder.zig:332-989). DESIGN.md §2.15.
// A wave takes 64 messages, in three passes:
//   1. lane per message: the checks and the framed length (sb_layout), status and length out;
//   2. the computed words (segment table, root pointer, every struct word) with (message, word)
//      flattened over the lanes, so a struct leaves as neighbouring 8-byte stores. A lane walks
//      the ops once: the walk gives the place of its word, folds the data writes that touch it
//      in program order and finds the allocation its pointer refers to;
//   3. per slice op, the rows (message, op) as a ragged copy in gather_kernel's piece scheme:
//      the aligned 16-byte chunks of the destination, rows of at most kGaShort bytes flattened
//      over the wave and longer rows a wave each. A row here is the content AND its tail (Text's
//      NUL, the padding to the word, a bit list's unused bits), written as zeros by the same
//      stores; rows begin and end at multiples of 8, so a piece is one 16-byte or one 8-byte store.
// Leans on:
//   common.h             kWave, kBlock, the ST_* statuses
//   device_helpers.h     lane_id, readlane, shfl_u64, wave_incl_sum, wave_lds_sync
//   struct_read.h        kGaShort
//   build_plan.h         SbPlan, SbOp, SbWord, sb_layout, sb_slice_words, sb_slice_elems, sb_elem_size
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "build_plan.h"
#include "kernels/common.h"
#include "kernels/device_helpers.h"
#include "kernels/struct_read.h"

namespace cpk {

// the op-major columns of one message
struct SbCols {
    const uint64_t* __restrict__ v;
    const uint64_t* __restrict__ l;
    const uint64_t* __restrict__ c;
    uint32_t n, m;
    __device__ __forceinline__ uint64_t value(uint32_t k) const { return v[(uint64_t)k * n + m]; }
    __device__ __forceinline__ uint64_t len(uint32_t k) const { return l[(uint64_t)k * n + m]; }
    __device__ __forceinline__ uint64_t count(uint32_t k) const { return c[(uint64_t)k * n + m]; }
};

// pieces of a row of `tot` bytes at dst (both multiples of 8)
__device__ __forceinline__ uint64_t build_pieces(uint64_t dst, uint64_t tot) {
    return tot ? ((dst + tot + 15) >> 4) - (dst >> 4) : 0;
}

// Piece p of a row: `clen` content bytes from src (any alignment), then zeros up to `tot`; the
// last content byte is ANDed with `msk` (a bit list's count). Only source chunks that hold a
// content byte of the piece are loaded (gather_piece's rule).
__device__ __forceinline__ void build_piece(uint64_t src, uint64_t dst, uint64_t clen, uint64_t tot, uint32_t msk,
                                            uint64_t p) {
    const uint64_t c16 = (dst & ~15ull) + 16 * p;
    const uint32_t lo = p == 0 ? (uint32_t)(dst & 15) : 0u;  // 0 or 8
    const uint64_t end = dst + tot, cend = dst + clen;
    const uint32_t hi = end - c16 < 16 ? (uint32_t)(end - c16) : 16u;  // 8 or 16
    // content bytes of the chunk are [lo, hc)
    const uint32_t hc = cend <= c16 ? 0u : (cend - c16 < 16 ? (uint32_t)(cend - c16) : 16u);
    const uint64_t t = src + (c16 - dst);  // wraps below src for b < lo: only bytes >= lo are used
    const uint64_t a = t & ~15ull;
    const uint32_t sh = (uint32_t)(t & 15);
    uint4 A = make_uint4(0, 0, 0, 0), B = A;
    if (hc > lo) {
        if (sh + lo < 16) A = *reinterpret_cast<const uint4*>(a);
        if (sh + hc > 16) B = *reinterpret_cast<const uint4*>(a + 16);
    }
    const uint64_t q0 = (uint64_t)A.x | ((uint64_t)A.y << 32), q1 = (uint64_t)A.z | ((uint64_t)A.w << 32);
    const uint64_t q2 = (uint64_t)B.x | ((uint64_t)B.y << 32), q3 = (uint64_t)B.z | ((uint64_t)B.w << 32);
    const uint64_t u0 = sh & 8 ? q1 : q0, u1 = sh & 8 ? q2 : q1, u2 = sh & 8 ? q3 : q2;
    const uint32_t s = (sh & 7) * 8;
    uint64_t x0 = s ? (u0 >> s) | (u1 << (64 - s)) : u0;
    uint64_t x1 = s ? (u1 >> s) | (u2 << (64 - s)) : u1;
    // the tail: bytes from hc on are zero
    if (hc <= 8) {
        x1 = 0;
        x0 = hc == 8 ? x0 : x0 & ((1ull << (8 * hc)) - 1);
    } else if (hc < 16) {
        x1 &= (1ull << (8 * (hc - 8))) - 1;
    }
    // a bit list's last byte, when it lies in this chunk
    if (msk != 0xFFu && hc > 0 && cend - c16 <= 16) {
        const uint32_t b = hc - 1;
        const uint64_t off_bits = (uint64_t)(0xFFu ^ msk) << (8 * (b & 7));
        if (b < 8) x0 &= ~off_bits;
        else x1 &= ~off_bits;
    }
    if (lo == 0 && hi == 16)
        *reinterpret_cast<uint4*>(c16) =
            make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
    else if (lo == 0)
        *reinterpret_cast<uint64_t*>(c16) = x0;
    else
        *reinterpret_cast<uint64_t*>(c16 + 8) = x1;
}

__global__ __launch_bounds__(kBlock) void build_fields_kernel(const uint8_t* __restrict__ pool, uint64_t pool_len,
                                                              uint32_t n, const SbPlan plan,
                                                              const uint64_t* __restrict__ value,
                                                              const uint64_t* __restrict__ len,
                                                              const uint64_t* __restrict__ count,
                                                              uint8_t* __restrict__ out,
                                                              const uint64_t* __restrict__ out_off,
                                                              const uint64_t* __restrict__ out_cap,
                                                              uint64_t* __restrict__ out_len,
                                                              int32_t* __restrict__ status) {
    __shared__ uint64_t s_src[kBlock], s_dst[kBlock];
    __shared__ uint32_t s_len[kBlock], s_tot[kBlock], s_msk[kBlock], s_pfx[kBlock];
    __shared__ uint32_t s_ok[kBlock];
    const uint32_t lane = lane_id();
    const uint32_t wbase = threadIdx.x - lane;  // this wave's slice of the arrays
    const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
    // ---- 1. lane per message: checks, length, status -------------------------------------------
    bool ok = false;
    uint64_t base = 0;  // the message's address
    if (row < n) {
        int32_t st = ST_OK;
        uint64_t olen = 0;
        if (out) {
            base = reinterpret_cast<uint64_t>(out) + out_off[row];
            if (base & 7) st = ST_ARG;
        }
        if (!st) {
            uint64_t segw = 0;
            st = sb_layout(plan, SbCols{value, len, count, n, row}, pool_len, &segw, nullptr);
            if (!st) {
                const uint64_t framed = 8 * (segw + 1);  // toBytes: one table word for one segment
                if (framed >= (1ull << 32)) st = ST_TOOLARGE;
                else if (out && framed > out_cap[row]) st = ST_SPACE;
                if (st == ST_OK || st == ST_SPACE) olen = framed;
            }
        }
        status[row] = st;
        out_len[row] = olen;
        ok = st == ST_OK;
    }
    if (!out) return;  // sizes only
    s_ok[threadIdx.x] = ok;
    wave_lds_sync();
    // ---- 2. the computed words, (message, word) over the lanes ---------------------------------
    const uint32_t first = blockIdx.x * kBlock + wbase;  // the wave's first message
    const uint32_t nmsg = first < n ? (n - first < (uint32_t)kWave ? n - first : (uint32_t)kWave) : 0u;
    const uint32_t nw = plan.n_words + 1;  // the segment-table word, then the plan's words
    for (uint32_t j = lane; j < nmsg * nw; j += kWave) {
        const uint32_t mi = j / nw, f = j - mi * nw;
        if (!s_ok[wbase + mi]) continue;
        const uint32_t m = first + mi;
        const SbCols col{value, len, count, n, m};
        const uint32_t pwi = f ? f - 1 : 0u;  // plan word
        const SbWord w = plan.word[pwi];
        const bool in_struct = f >= 2;
        const bool is_ptr = in_struct && w.is_ptr;
        uint64_t cur = 1, mypos = 0, val = 0;
        uint64_t tstart = 0, tcount = 0;
        uint32_t tkind = 0;  // 0: null, 1: struct, 2: list
        uint32_t tdw = 0, tpw = 0, tes = 0;
        for (uint32_t k = 0; k < plan.n_ops; ++k) {
            const SbOp o = plan.op[k];
            if (in_struct && k == w.owner) mypos = cur + w.local;
            if (o.what == SB_STRUCT) {
                if (is_ptr && k == w.ptr_op && o.swords) {
                    tkind = 1, tstart = cur, tdw = o.dw, tpw = o.pw;
                }
                cur += o.swords;
            } else if (o.what == SB_SLICE) {
                const uint64_t L = col.len(k);
                if (L == CAPNP_PACKED_BUILD_ABSENT) continue;
                if (is_ptr && k == w.ptr_op) {
                    tkind = 2, tstart = cur, tes = sb_elem_size(o.kind);
                    tcount = sb_slice_elems(o.kind, L, o.kind == CAPNP_PACKED_FIELD_LIST_BIT ? col.count(k) : 0);
                }
                cur += sb_slice_words(o.kind, L);
            } else if (o.what != SB_NONE && in_struct && !w.is_ptr) {
                const uint32_t d = pwi - o.word;  // 0: the write's first word, 1: its second
                const bool second = d == 1 && o.what == SB_DATA && o.shift + o.width > 8u;
                if (d != 0 && !second) continue;
                if (col.len(k) == CAPNP_PACKED_BUILD_ABSENT) continue;
                const uint64_t v = col.value(k);
                if (o.what == SB_BOOL) {  // struct_builder.zig:449-458
                    const uint32_t bp = 8u * o.shift + o.width;
                    val = (val & ~(1ull << bp)) | ((v & 1) << bp);
                } else {  // :356-430, little-endian
                    const uint64_t wm = o.width == 8 ? ~0ull : (1ull << (8u * o.width)) - 1;
                    if (!second) {
                        const uint32_t s = 8u * o.shift;
                        val = (val & ~(wm << s)) | ((v & wm) << s);
                    } else {
                        const uint32_t s = 8u * (8u - o.shift);  // shift >= 1 here
                        val = (val & ~(wm >> s)) | ((v & wm) >> s);
                    }
                }
            }
        }
        uint64_t at = 0;  // the word's place in the framed message, in words
        if (f == 0) {
            val = cur << 32;  // toBytes (message.zig:2147-2157): segment count - 1 = 0, then segment 0's words
        } else if (f == 1) {
            at = 1;  // allocateStruct's root pointer (:2076-2087): offset 0
            val = ((uint64_t)plan.op[0].dw << 32) | ((uint64_t)plan.op[0].pw << 48);
        } else {
            at = 1 + mypos;
            if (is_ptr) {
                const uint64_t off = (tstart - mypos - 1) & 0x3FFFFFFFull;  // message.zig:1808-1811, :1872-1875, :1943-1946
                val = tkind == 1   ? (off << 2) | ((uint64_t)tdw << 32) | ((uint64_t)tpw << 48)
                      : tkind == 2 ? 1ull | (off << 2) | ((uint64_t)tes << 32) | (tcount << 35)
                                   : 0ull;
            }
        }
        *reinterpret_cast<uint64_t*>(reinterpret_cast<uint64_t>(out) + out_off[m] + 8 * at) = val;
    }
    // ---- 3. the slices, op by op ----------------------------------------------------------------
    uint64_t cur = 1;
    for (uint32_t k = 0; k < plan.n_ops; ++k) {
        const SbOp o = plan.op[k];
        if (o.what == SB_STRUCT) cur += o.swords;
        if (o.what != SB_SLICE) continue;
        uint64_t src = 0, dst = 0;
        uint32_t clen = 0, tot = 0, msk = 0xFFu;
        if (ok) {
            const uint64_t L = len[(uint64_t)k * n + row];
            if (L != CAPNP_PACKED_BUILD_ABSENT) {
                clen = (uint32_t)L;  // below 2^32: the count is below 2^29
                tot = (uint32_t)(sb_slice_words(o.kind, L) << 3);
                src = reinterpret_cast<uint64_t>(pool) + value[(uint64_t)k * n + row];
                dst = base + 8 * (1 + cur);
                if (o.kind == CAPNP_PACKED_FIELD_LIST_BIT) {
                    const uint32_t r = (uint32_t)count[(uint64_t)k * n + row] & 7u;
                    if (r) msk = (1u << r) - 1;
                }
                cur += tot >> 3;
            }
        }
        // short rows, flattened
        const bool is_short = tot <= kGaShort;
        const uint32_t np = is_short ? (uint32_t)build_pieces(dst, tot) : 0u;
        const uint32_t incl = wave_incl_sum(np);
        const uint32_t total = readlane(incl, kWave - 1);
        wave_lds_sync();  // the previous op's reads are done
        s_src[threadIdx.x] = src;
        s_dst[threadIdx.x] = dst;
        s_len[threadIdx.x] = clen;
        s_tot[threadIdx.x] = is_short ? tot : 0u;
        s_msk[threadIdx.x] = msk;
        s_pfx[threadIdx.x] = incl;
        wave_lds_sync();
        for (uint32_t j = lane; j < total; j += kWave) {
            uint32_t r = 0;  // the first row with pfx[r] > j
#pragma unroll
            for (uint32_t step = kWave / 2; step; step >>= 1)
                if (s_pfx[wbase + r + step - 1] <= j) r += step;
            const uint32_t before = r ? s_pfx[wbase + r - 1] : 0u;
            build_piece(s_src[wbase + r], s_dst[wbase + r], s_len[wbase + r], s_tot[wbase + r], s_msk[wbase + r],
                        j - before);
        }
        // long rows, a wave each
        uint64_t longs = __ballot(!is_short);
        while (longs) {
            const uint32_t r = (uint32_t)__builtin_ctzll(longs);
            longs &= longs - 1;
            const uint64_t rs = shfl_u64(src, r), rd = shfl_u64(dst, r);
            const uint64_t rl = (uint32_t)__shfl((int)clen, (int)r, kWave), rt = (uint32_t)__shfl((int)tot, (int)r, kWave);
            const uint32_t rm = (uint32_t)__shfl((int)msk, (int)r, kWave);
            const uint64_t pieces = build_pieces(rd, rt);
            for (uint64_t p = lane; p < pieces; p += kWave) build_piece(rs, rd, rl, rt, rm, p);
        }
    }
}

}  // namespace cpk
