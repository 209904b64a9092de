// kernels/message_walk.h
// The walk of a decoded message that read_fields_kernel (struct_read.h), list_heads_kernel and
// read_elements_kernel (list_read.h) share, each piece once: Message.init's
// front with the segment bounds in an LDS column of the lane (mw_init, MwSegsLds), getRootStruct
// (mw_root), resolvePointer / resolveStructPointer / resolveListPointer and readStruct (mw_resolve,
// mw_resolve_struct, mw_resolve_list, mw_step), one field of a struct (mw_read_field), the loop
// over a descriptor table (mw_read_fields) and the LDS staging of its results (MwStage). The
// pointer functions are templates over the way a kernel looks a segment up (a Segs: d, nseg(),
// lookup()). Line numbers are message.zig's.
// Leans on:
//   common.h             kBlock, kMsgMaxSegs, the ST_* statuses, capnp_packed_field
//   device_helpers.h     gload64, ptr_offset_words
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"

namespace cpk {

constexpr uint32_t kSrSegs = 4;         // segments whose bounds a lane keeps in LDS
constexpr uint32_t kSrGroup = 4;        // fields whose results go out together
constexpr uint32_t kSrFarDepth = 8;     // resolvePointer's depth (message.zig:493/526)

// The descriptors as a kernel argument (wave-uniform: scalar loads); `same` has bit f set when
// field f's path is field f - 1's, so a struct is resolved once for a run of fields that share it.
struct SrFields {
    capnp_packed_field f[CAPNP_PACKED_MAX_FIELDS];
    uint32_t same;
};

struct MwResolved {  // resolvePointer's result (:451-490)
    uint32_t seg;
    uint64_t pos, word, over;
    bool has_over;
};

struct MwStruct {
    uint32_t seg;
    uint64_t soff;  // the segment's offset in the message
    uint64_t off;   // the struct's offset in its segment
    uint32_t dw, pc;
};

struct MwList {  // resolveListPointer's result: the content and its byte length
    uint32_t seg, es;
    uint64_t soff, slen, co, cnt, bytes;
};

struct MwResult {  // one field's
    int32_t st;
    uint64_t v, l, c;
};

// entry e of the message's segment table (entry 0 the count, entry s + 1 segment s's words)
__device__ __forceinline__ uint32_t mw_entry_at(const uint8_t* d, uint32_t e) {
    const uint64_t w = gload64(d + 4ull * (e & ~1u));
    return (e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
}

// Segment lookup after mw_init: segment s < kSrSegs is [segb[s], segb[s + 1]) of the message, a
// column per lane in LDS, as in validate_kernel (in registers the compiler turns the lookup into a
// table in scratch); the others by a walk of the table.
struct MwSegsLds {
    const uint8_t* d;
    uint32_t n;
    const uint32_t* segb;  // bound i at segb[i * kBlock]
    __device__ __forceinline__ uint32_t nseg() { return n; }
    __device__ __forceinline__ void lookup(uint32_t s, uint64_t& off, uint64_t& slen) {
        if (s < kSrSegs) {
            off = segb[kBlock * s];
            slen = segb[kBlock * (s + 1)] - off;
            return;
        }
        uint64_t acc = segb[kBlock * kSrSegs];
        for (uint32_t i = kSrSegs; i < s; ++i) acc += 8ull * mw_entry_at(d, i + 1);
        off = acc;
        slen = 8ull * mw_entry_at(d, s + 1);
    }
};

// ---- Message.init (:341-394), message_init_kernel's statuses: the message is `len` bytes at d,
// moff bytes into its buffer; fills the lane's column segb and the segment count ---------------
__device__ __forceinline__ int32_t mw_init(const uint8_t* d, uint64_t moff, uint64_t len, uint32_t* segb,
                                           uint32_t& nseg) {
    if ((moff & 7) || len >= (1ull << 32)) return ST_ARG;
    if (len < 4) return ST_EOS;
    uint64_t w = len >= 8 ? gload64(d) : (uint64_t)*reinterpret_cast<const uint32_t*>(d);
    const uint32_t m1 = (uint32_t)w;
    if (m1 == 0xFFFFFFFFu) return ST_SEGCOUNT;
    if ((uint64_t)m1 + 1 > kMsgMaxSegs) return ST_SEGLIMIT;
    nseg = m1 + 1;
    const uint64_t header = 4ull * (1 + nseg + ((nseg & 1) ? 0 : 1));
    if (header > len) return ST_TRUNC;
    uint64_t acc = header;
    segb[0] = (uint32_t)header;
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint32_t e = s + 1;  // the table entry, given the word last read
        if ((e & 1) == 0) w = gload64(d + 4ull * e);
        acc += 8ull * ((e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w);
        if (acc > len) return ST_TRUNC;  // :380
        if (s < kSrSegs) segb[kBlock * (s + 1)] = (uint32_t)acc;
    }
    return ST_OK;
}

// ---- resolvePointer (:451-490) ---------------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t mw_resolve(Segs& sg, MwResolved& r) {
    r.has_over = false;
    r.over = 0;
    for (uint32_t depth = kSrFarDepth;; --depth) {
        if (depth == 0) return ST_NEST;  // PointerDepthLimit
        if ((r.word & 3) != 2) return ST_OK;
        const bool dbl = (r.word >> 2) & 1;
        const uint64_t lpos = ((r.word >> 3) & 0x1FFFFFFFull) * 8;
        const uint32_t fseg = (uint32_t)(r.word >> 32);
        if (fseg >= sg.nseg()) return ST_SEGID;  // :431
        uint64_t so, sl;
        sg.lookup(fseg, so, sl);
        if (lpos + (dbl ? 16 : 8) > sl) return ST_OOB;  // :435
        const uint64_t landing = gload64(sg.d + so + lpos);
        if (!dbl) {
            r.seg = fseg;
            r.pos = lpos;
            r.word = landing;
            continue;
        }
        const uint64_t tag = gload64(sg.d + so + lpos + 8);
        if ((landing & 3) != 2 || ((landing >> 2) & 1)) return ST_FAR;  // :478/:480
        if ((uint32_t)(landing >> 32) >= sg.nseg()) return ST_SEGID;    // :481
        r.seg = (uint32_t)(landing >> 32);
        r.pos = 0;
        r.word = tag;
        r.has_over = true;
        r.over = ((landing >> 3) & 0x1FFFFFFFull) * 8;
        return ST_OK;
    }
}

// ---- resolveStructPointer (:492-523) -----------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t mw_resolve_struct(Segs& sg, uint32_t seg, uint64_t pos, uint64_t word,
                                                     MwStruct& s) {
    MwResolved r{seg, pos, word, 0, false};
    if (int32_t st = mw_resolve(sg, r)) return st;
    if (r.word == 0 || (r.word & 3) != 0) return ST_PTR;  // InvalidRootPointer
    int64_t o = (int64_t)r.pos + 8 + ptr_offset_words(r.word) * 8;
    if (r.has_over) o = (int64_t)r.over;
    if (o < 0) return ST_PTR;
    const uint32_t dw = (uint32_t)(r.word >> 32) & 0xFFFFu, pc = (uint32_t)(r.word >> 48);
    uint64_t so, sl;
    sg.lookup(r.seg, so, sl);
    if ((uint64_t)o + 8ull * (dw + pc) > sl) return ST_TRUNC;  // :514
    s = MwStruct{r.seg, so, (uint64_t)o, dw, pc};
    return ST_OK;
}

// ---- getRootStruct (:973-985) ------------------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t mw_root(Segs& sg, MwStruct& root) {
    uint64_t so, sl;
    sg.lookup(0, so, sl);
    if (sl < 8) return ST_TRUNC;
    return mw_resolve_struct(sg, 0, 0, gload64(sg.d + so), root);
}

// ---- readStruct (:1224-1235) -------------------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t mw_step(Segs& sg, MwStruct& cur, uint32_t pi) {
    if (pi >= cur.pc) return ST_OOB;
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * pi;
    const uint64_t word = gload64(sg.d + cur.soff + ppos);
    if (word == 0) return ST_PTR;
    MwStruct next{};
    const int32_t st = mw_resolve_struct(sg, cur.seg, ppos, word, next);
    if (st == ST_OK) cur = next;
    return st;
}

// ---- resolveListPointer (:525-561) of a non-null word ------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t mw_resolve_list(Segs& sg, uint32_t seg, uint64_t pos, uint64_t word,
                                                   MwList& L) {
    MwResolved r{seg, pos, word, 0, false};
    if (int32_t st = mw_resolve(sg, r)) return st;
    if (r.word == 0 || (r.word & 3) != 1) return ST_PTR;
    const uint32_t es = (uint32_t)(r.word >> 32) & 7u;
    const uint64_t cnt = r.word >> 35;
    int64_t co = (int64_t)r.pos + 8 + ptr_offset_words(r.word) * 8;
    if (r.has_over) co = (int64_t)r.over;
    if (co < 0) return ST_OOB;  // :447
    const uint64_t bytes = es == 0 ? 0 : es == 1 ? (cnt + 7) / 8 : es == 2 ? cnt : es == 3 ? 2 * cnt
                         : es == 4 ? 4 * cnt : es == 7 ? 8 * (cnt + 1) : 8 * cnt;
    uint64_t so, sl;
    sg.lookup(r.seg, so, sl);
    if ((uint64_t)co + bytes > sl) return ST_OOB;  // :553
    L = MwList{r.seg, es, so, sl, (uint64_t)co, cnt, bytes};
    return ST_OK;
}

// ---- one field of a struct: the data section reads (:1051-1158) and the slice reads
// (resolveListPointerAt :1187-1198, the typed reads :1259-1415, readText :1417-1443). Every load
// is an aligned 8-byte word of one of the message's segments. ------------------------------------
template <class Segs>
__device__ __forceinline__ MwResult mw_read_field(Segs& sg, uint64_t moff, const MwStruct& cur,
                                                  const capnp_packed_field& F) {
    if (F.kind <= CAPNP_PACKED_FIELD_BOOL) {
        const uint32_t width = F.kind == CAPNP_PACKED_FIELD_U64 ? 8u : F.kind == CAPNP_PACKED_FIELD_U32 ? 4u
                             : F.kind == CAPNP_PACKED_FIELD_U16 ? 2u : 1u;
        if ((uint64_t)F.offset + width > 8ull * cur.dw) return MwResult{ST_OK, 0, 0, 0};
        const uint8_t* const p = sg.d + cur.soff + cur.off + (F.offset & ~7u);
        const uint32_t sh = (F.offset & 7u) * 8u;
        uint64_t v = gload64(p) >> sh;
        if ((F.offset & 7u) + width > 8u) v |= gload64(p + 8) << (64u - sh);  // sh > 0 here
        if (width < 8) v &= (1ull << (8 * width)) - 1;
        if (F.kind == CAPNP_PACKED_FIELD_BOOL) v = (v >> F.bit) & 1;
        return MwResult{ST_OK, v, width, 1};
    }
    const bool text = F.kind == CAPNP_PACKED_FIELD_TEXT;
    if (F.offset >= cur.pc) return MwResult{text ? ST_OK : ST_OOB, 0, 0, 0};
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * F.offset;
    const uint64_t word = gload64(sg.d + cur.soff + ppos);
    if (word == 0) return MwResult{text ? ST_OK : ST_PTR, 0, 0, 0};
    MwList L{};
    if (int32_t st = mw_resolve_list(sg, cur.seg, ppos, word, L)) return MwResult{st, 0, 0, 0};
    const uint32_t want = (text || F.kind == CAPNP_PACKED_FIELD_DATA) ? 2u
                        : F.kind == CAPNP_PACKED_FIELD_LIST_BIT ? 1u
                        : F.kind - CAPNP_PACKED_FIELD_LIST_16 + 3u;
    if (L.es != want) return MwResult{ST_PTR, 0, 0, 0};  // :1261 ..., InvalidTextPointer :1432
    uint64_t l = L.bytes, c = L.cnt;
    if (text && L.cnt) {  // one trailing NUL is not part of the text (:1439)
        const uint64_t last = L.co + L.cnt - 1;
        if (((gload64(sg.d + L.soff + (last & ~7ull)) >> (8 * (last & 7))) & 0xFF) == 0) {
            --l;
            --c;
        }
    }
    return MwResult{ST_OK, moff + L.soff + L.co, l, c};
}

// ---- the results' way out. Field f of the lane goes to [f * stride + row] of the four columns
// (`count` may be null). A field's results wait in LDS (4 dwords: the value, the length, and the
// count or, with the top bit set, the status: lengths are below 4 GiB, counts below 2^29) and go
// out a group of fields at a time, so no store stands between a group's dependent loads (on gfx9
// a load's vmcnt wait also waits for the stores issued before it). Worth 4% on read_fields_kernel's
// measured shape. -----------------------------------------------------------------------------------
struct MwStage {
    uint32_t* res;  // the lane's slice: dword i of its field g at res[(4 g + i) * kBlock]
    uint64_t row, stride;
    uint64_t* value;
    uint64_t* flen;
    uint64_t* count;
    int32_t* status;
    __device__ __forceinline__ void store(uint32_t f, int32_t st, uint64_t v, uint64_t l, uint64_t c) const {
        const uint64_t at = (uint64_t)f * stride + row;
        value[at] = v;
        flen[at] = l;
        if (count) count[at] = c;
        status[at] = st;
    }
    __device__ __forceinline__ void store_all(uint32_t n_fields, int32_t st) const {  // no field was read
        for (uint32_t f = 0; f < n_fields; ++f) store(f, st, 0, 0, 0);
    }
    __device__ __forceinline__ void put(uint32_t f, const MwResult& r) const {
        uint32_t* const q = res + 4 * kBlock * (f % kSrGroup);
        q[0] = (uint32_t)r.v;
        q[kBlock] = (uint32_t)(r.v >> 32);
        q[2 * kBlock] = (uint32_t)r.l;
        q[3 * kBlock] = r.st == ST_OK ? (uint32_t)r.c : 0x80000000u | (uint32_t)r.st;
    }
    __device__ __forceinline__ void flush(uint32_t f0, uint32_t f1) const {  // fields [f0, f1) of one group
        for (uint32_t f = f0; f < f1; ++f) {
            const uint32_t* const q = res + 4 * kBlock * (f % kSrGroup);
            const uint32_t cs = q[3 * kBlock];
            const bool ok = !(cs >> 31);
            store(f, ok ? ST_OK : (int32_t)(cs & 0x7FFFFFFFu), (uint64_t)q[0] | ((uint64_t)q[kBlock] << 32),
                  q[2 * kBlock], ok ? cs : 0u);
        }
    }
};

// ---- every field of a descriptor table (n_fields >= 1), from the struct `top`: readStruct along
// the field's path unless it is the field before's, then the field ------------------------------
template <class Segs>
__device__ __forceinline__ void mw_read_fields(Segs& sg, uint64_t moff, const MwStruct& top, const SrFields& fs,
                                               uint32_t n_fields, const MwStage& out) {
    MwStruct cur = top;
    int32_t cur_st = ST_OK;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (f && f % kSrGroup == 0) out.flush(f - kSrGroup, f);
        const capnp_packed_field& F = fs.f[f];
        if (!((fs.same >> f) & 1)) {
            cur = top;
            cur_st = ST_OK;
            for (uint32_t k = 0; k < F.path_len && cur_st == ST_OK; ++k) cur_st = mw_step(sg, cur, F.path[k]);
        }
        if (cur_st != ST_OK) { out.put(f, MwResult{cur_st, 0, 0, 0}); continue; }
        out.put(f, mw_read_field(sg, moff, cur, F));
    }
    out.flush((n_fields - 1) / kSrGroup * kSrGroup, n_fields);
}

}  // namespace cpk
