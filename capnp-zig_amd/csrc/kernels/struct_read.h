// kernels/struct_read.h
// Reads on decoded messages: read_fields_kernel (getRootStruct, readStruct along a path, the
// scalar and slice reads of StructReader as columns, lane per message) and gather_kernel (the
// slices as dense bytes, a ragged byte copy). DESIGN.md §2.13.
// Leans on:
//   common.h             kWave, kBlock, kMsgMaxSegs, the ST_* statuses, capnp_packed_field
//   device_helpers.h     gload64, ptr_offset_words, wave_incl_sum, wave_lds_sync, store_partial16
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"

namespace cpk {

// ---------------------------------------------------------------------------
// read_fields_kernel: message.zig:973-985 (getRootStruct), :451-561 (resolvePointer,
// resolveStructPointer, resolveListPointer), :1051-1158 (data reads), :1187-1198, :1224-1235,
// :1259-1443 (readStruct, the slice reads, readText), lane per message, every field of the
// message in turn. The descriptors are kernel arguments (wave-uniform: scalar loads); `same`
// has bit f set when field f's path is field f - 1's, so a struct is resolved once for a run
// of fields that share it. Every load is an aligned 8-byte word of the message's segment table
// or of one of its segments.
// ---------------------------------------------------------------------------
constexpr uint32_t kSrSegs = 4;         // segments whose bounds a lane keeps in LDS
constexpr uint32_t kSrGroup = 4;        // fields whose results go out together
constexpr uint32_t kSrFarDepth = 8;     // resolvePointer's depth (message.zig:493/526)

struct SrFields {
    capnp_packed_field f[CAPNP_PACKED_MAX_FIELDS];
    uint32_t same;
};

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

    // A field's results wait in LDS (4 dwords: the value, the length, and the count or, with the
    // top bit set, the status: lengths are below 4 GiB, counts below 2^29) and go out a group of
    // fields at a time, so no store stands between a group's dependent loads (on gfx9 a load's
    // vmcnt wait also waits for the stores issued before it). Worth 4% on the measured shape.
    uint32_t* const res = res_all + threadIdx.x;
    auto store = [&](uint32_t f, int32_t st, uint64_t v, uint64_t l, uint64_t c) {
        const uint64_t at = (uint64_t)f * n + msg;
        value[at] = v;
        flen[at] = l;
        if (count) count[at] = c;
        status[at] = st;
    };
    auto put = [&](uint32_t f, int32_t st, uint64_t v, uint64_t l, uint64_t c) {
        uint32_t* const r = res + 4 * kBlock * (f % kSrGroup);
        r[0] = (uint32_t)v;
        r[kBlock] = (uint32_t)(v >> 32);
        r[2 * kBlock] = (uint32_t)l;
        r[3 * kBlock] = st == ST_OK ? (uint32_t)c : 0x80000000u | (uint32_t)st;
    };
    auto flush = [&](uint32_t f0, uint32_t f1) {  // fields [f0, f1) of one group
        for (uint32_t f = f0; f < f1; ++f) {
            const uint32_t* const r = res + 4 * kBlock * (f % kSrGroup);
            const uint32_t cs = r[3 * kBlock];
            const bool ok = !(cs >> 31);
            store(f, ok ? ST_OK : (int32_t)(cs & 0x7FFFFFFFu), (uint64_t)r[0] | ((uint64_t)r[kBlock] << 32),
                  r[2 * kBlock], ok ? cs : 0u);
        }
    };
    auto fail_all = [&](int32_t st) {
        for (uint32_t f = 0; f < n_fields; ++f) store(f, st, 0, 0, 0);
    };

    // ---- Message.init (:341-394), message_init_kernel's statuses ---------------------------
    if ((moff & 7) || len >= (1ull << 32)) return fail_all(ST_ARG);
    if (len < 4) return fail_all(ST_EOS);
    const uint64_t w0 = len >= 8 ? gload64(d) : (uint64_t)*reinterpret_cast<const uint32_t*>(d);
    const uint32_t m1 = (uint32_t)w0;
    if (m1 == 0xFFFFFFFFu) return fail_all(ST_SEGCOUNT);
    if ((uint64_t)m1 + 1 > kMsgMaxSegs) return fail_all(ST_SEGLIMIT);
    const uint32_t nseg = m1 + 1;
    const uint64_t header = 4ull * (1 + nseg + ((nseg & 1) ? 0 : 1));
    if (header > len) return fail_all(ST_TRUNC);
    // table entry e (entry 0 the count, entry s + 1 segment s's words), given the word last read
    auto entry = [&](uint32_t e, uint64_t& w) {
        if ((e & 1) == 0) w = gload64(d + 4ull * e);
        return (e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
    };
    auto entry_at = [&](uint32_t e) {  // the same by a load of its own
        const uint64_t w = gload64(d + 4ull * (e & ~1u));
        return (e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
    };
    // segment s < kSrSegs is [segb[s], segb[s + 1]) of the message: a column per lane in LDS, as
    // in validate_kernel (in registers the compiler turns the lookup into a table in scratch)
    uint32_t* const segb = segb_all + threadIdx.x;
    {
        uint64_t w = w0, acc = header;
        segb[0] = (uint32_t)header;
        for (uint32_t s = 0; s < nseg; ++s) {
            acc += 8ull * entry(s + 1, w);
            if (acc > len) return fail_all(ST_TRUNC);  // :380
            if (s < kSrSegs) segb[kBlock * (s + 1)] = (uint32_t)acc;
        }
    }
    // segment s < nseg: its offset in the message and its length
    auto seg_lookup = [&](uint32_t s, uint64_t& off, uint64_t& slen) {
        if (s < kSrSegs) {
            off = segb[kBlock * s];
            slen = segb[kBlock * (s + 1)] - off;
            return;
        }
        uint64_t acc = segb[kBlock * kSrSegs];
        for (uint32_t i = kSrSegs; i < s; ++i) acc += 8ull * entry_at(i + 1);
        off = acc;
        slen = 8ull * entry_at(s + 1);
    };

    // ---- resolvePointer (:451-490) ---------------------------------------------------------
    struct Resolved {
        uint32_t seg;
        uint64_t pos, word, over;
        bool has_over;
    };
    auto resolve = [&](Resolved& r) -> int32_t {
        r.has_over = false;
        r.over = 0;
        for (uint32_t depth = kSrFarDepth;; --depth) {
            if (depth == 0) return ST_NEST;  // PointerDepthLimit
            if ((r.word & 3) != 2) return ST_OK;
            const bool dbl = (r.word >> 2) & 1;
            const uint64_t lpos = ((r.word >> 3) & 0x1FFFFFFFull) * 8;
            const uint32_t fseg = (uint32_t)(r.word >> 32);
            if (fseg >= nseg) return ST_SEGID;  // :431
            uint64_t so, sl;
            seg_lookup(fseg, so, sl);
            if (lpos + (dbl ? 16 : 8) > sl) return ST_OOB;  // :435
            const uint64_t landing = gload64(d + so + lpos);
            if (!dbl) {
                r.seg = fseg;
                r.pos = lpos;
                r.word = landing;
                continue;
            }
            const uint64_t tag = gload64(d + so + lpos + 8);
            if ((landing & 3) != 2 || ((landing >> 2) & 1)) return ST_FAR;  // :478/:480
            if ((uint32_t)(landing >> 32) >= nseg) return ST_SEGID;       // :481
            r.seg = (uint32_t)(landing >> 32);
            r.pos = 0;
            r.word = tag;
            r.has_over = true;
            r.over = ((landing >> 3) & 0x1FFFFFFFull) * 8;
            return ST_OK;
        }
    };

    // ---- resolveStructPointer (:492-523) ----------------------------------------------------
    struct Struct {
        uint32_t seg;
        uint64_t soff;  // the segment's offset in the message
        uint64_t off;   // the struct's offset in its segment
        uint32_t dw, pc;
    };
    auto resolve_struct = [&](uint32_t seg, uint64_t pos, uint64_t word, Struct& s) -> int32_t {
        Resolved r{seg, pos, word, 0, false};
        if (int32_t st = resolve(r)) return st;
        if (r.word == 0 || (r.word & 3) != 0) return ST_PTR;  // InvalidRootPointer
        int64_t o = (int64_t)r.pos + 8 + ptr_offset_words(r.word) * 8;
        if (r.has_over) o = (int64_t)r.over;
        if (o < 0) return ST_PTR;
        const uint32_t dw = (uint32_t)(r.word >> 32) & 0xFFFFu, pc = (uint32_t)(r.word >> 48);
        uint64_t so, sl;
        seg_lookup(r.seg, so, sl);
        if ((uint64_t)o + 8ull * (dw + pc) > sl) return ST_TRUNC;  // :514
        s = Struct{r.seg, so, (uint64_t)o, dw, pc};
        return ST_OK;
    };

    // ---- getRootStruct (:973-985) ------------------------------------------------------------
    Struct root{};
    {
        uint64_t so, sl;
        seg_lookup(0, so, sl);
        if (sl < 8) return fail_all(ST_TRUNC);
        if (int32_t st = resolve_struct(0, 0, gload64(d + so), root)) return fail_all(st);
    }

    Struct cur = root;
    int32_t cur_st = ST_OK;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (f && f % kSrGroup == 0) flush(f - kSrGroup, f);
        const capnp_packed_field& F = fs.f[f];
        if (!((fs.same >> f) & 1)) {  // readStruct along the path (:1224-1235)
            cur = root;
            cur_st = ST_OK;
            for (uint32_t k = 0; k < F.path_len && cur_st == ST_OK; ++k) {
                const uint32_t pi = F.path[k];
                if (pi >= cur.pc) { cur_st = ST_OOB; break; }
                const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * pi;
                const uint64_t word = gload64(d + cur.soff + ppos);
                if (word == 0) { cur_st = ST_PTR; break; }
                Struct next{};
                cur_st = resolve_struct(cur.seg, ppos, word, next);
                if (cur_st == ST_OK) cur = next;
            }
        }
        if (cur_st != ST_OK) { put(f, cur_st, 0, 0, 0); continue; }

        if (F.kind <= CAPNP_PACKED_FIELD_BOOL) {  // the data section reads (:1051-1158)
            const uint32_t width = F.kind == CAPNP_PACKED_FIELD_U64 ? 8u : F.kind == CAPNP_PACKED_FIELD_U32 ? 4u
                                 : F.kind == CAPNP_PACKED_FIELD_U16 ? 2u : 1u;
            if ((uint64_t)F.offset + width > 8ull * cur.dw) { put(f, ST_OK, 0, 0, 0); continue; }
            const uint8_t* const p = d + cur.soff + cur.off + (F.offset & ~7u);
            const uint32_t sh = (F.offset & 7u) * 8u;
            uint64_t v = gload64(p) >> sh;
            if ((F.offset & 7u) + width > 8u) v |= gload64(p + 8) << (64u - sh);  // sh > 0 here
            if (width < 8) v &= (1ull << (8 * width)) - 1;
            if (F.kind == CAPNP_PACKED_FIELD_BOOL) v = (v >> F.bit) & 1;
            put(f, ST_OK, v, width, 1);
            continue;
        }

        // the slice reads: resolveListPointerAt (:1187-1198), readText's front (:1417-1429)
        const bool text = F.kind == CAPNP_PACKED_FIELD_TEXT;
        if (F.offset >= cur.pc) { put(f, text ? ST_OK : ST_OOB, 0, 0, 0); continue; }
        const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * F.offset;
        Resolved r{cur.seg, ppos, gload64(d + cur.soff + ppos), 0, false};
        if (r.word == 0) { put(f, text ? ST_OK : ST_PTR, 0, 0, 0); continue; }
        // resolveListPointer (:525-561)
        if (int32_t st = resolve(r)) { put(f, st, 0, 0, 0); continue; }
        if (r.word == 0 || (r.word & 3) != 1) { put(f, ST_PTR, 0, 0, 0); continue; }
        const uint32_t es = (uint32_t)(r.word >> 32) & 7u;
        const uint64_t cnt = r.word >> 35;
        int64_t co = (int64_t)r.pos + 8 + ptr_offset_words(r.word) * 8;
        if (r.has_over) co = (int64_t)r.over;
        if (co < 0) { put(f, ST_OOB, 0, 0, 0); continue; }  // :447
        const uint64_t bytes = es == 0 ? 0 : es == 1 ? (cnt + 7) / 8 : es == 2 ? cnt : es == 3 ? 2 * cnt
                             : es == 4 ? 4 * cnt : es == 7 ? 8 * (cnt + 1) : 8 * cnt;
        uint64_t so, sl;
        seg_lookup(r.seg, so, sl);
        if ((uint64_t)co + bytes > sl) { put(f, ST_OOB, 0, 0, 0); continue; }  // :553
        const uint32_t want = (text || F.kind == CAPNP_PACKED_FIELD_DATA) ? 2u
                            : F.kind == CAPNP_PACKED_FIELD_LIST_BIT ? 1u
                            : F.kind - CAPNP_PACKED_FIELD_LIST_16 + 3u;
        if (es != want) { put(f, ST_PTR, 0, 0, 0); continue; }  // :1261 ..., InvalidTextPointer :1432
        uint64_t l = bytes, c = cnt;
        if (text && cnt) {  // one trailing NUL is not part of the text (:1439)
            const uint64_t last = (uint64_t)co + cnt - 1;
            if (((gload64(d + so + (last & ~7ull)) >> (8 * (last & 7))) & 0xFF) == 0) {
                --l;
                --c;
            }
        }
        put(f, ST_OK, moff + so + (uint64_t)co, l, c);
    }
    flush((n_fields - 1) / kSrGroup * kSrGroup, n_fields);
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
