// kernels/list_read.h
// Struct lists and pointer lists of decoded messages as element tables:
// list_heads_kernel (one list per message: readStructList / readTextList / readPointerList, lane
// per message) and read_elements_kernel (fields of every element of every list as columns, lane
// per element).
// The pointer resolution and the field body are __device__ templates here (lr_resolve,
// lr_resolve_struct, lr_read_field), over the way a kernel looks a segment up. They restate the
// lambdas inside read_fields_kernel (struct_read.h), which stays as it is so that its code does
// not move: the duplication is named in DESIGN.md §2.14 for a later tidy-up.
// Leans on:
//   common.h             kBlock, kMsgMaxSegs, the ST_* statuses, capnp_packed_field / _list_head
//   device_helpers.h     gload64, ptr_offset_words
//   struct_read.h        kSrSegs, kSrGroup, kSrFarDepth, SrFields
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"
#include "kernels/struct_read.h"

namespace cpk {

struct LrResolved {  // resolvePointer's result (message.zig:451-490)
    uint32_t seg;
    uint64_t pos, word, over;
    bool has_over;
};

struct LrStruct {
    uint32_t seg;
    uint64_t soff;  // the segment's offset in the message
    uint64_t off;   // the struct's offset in its segment
    uint32_t dw, pc;
};

// Segment lookup of list_heads_kernel: the bounds of the first kSrSegs segments in an LDS column
// of the lane (read_fields_kernel's arrangement), the others by a walk of the table.
struct LrSegsLds {
    const uint8_t* d;
    uint32_t n;
    const uint32_t* segb;  // bound i at segb[i * kBlock]
    __device__ __forceinline__ uint32_t nseg() { return n; }
    __device__ __forceinline__ uint32_t entry_at(uint32_t e) const {
        const uint64_t w = gload64(d + 4ull * (e & ~1u));
        return (e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
    }
    __device__ __forceinline__ void lookup(uint32_t s, uint64_t& off, uint64_t& slen) {
        if (s < kSrSegs) {
            off = segb[kBlock * s];
            slen = segb[kBlock * (s + 1)] - off;
            return;
        }
        uint64_t acc = segb[kBlock * kSrSegs];
        for (uint32_t i = kSrSegs; i < s; ++i) acc += 8ull * entry_at(i + 1);
        off = acc;
        slen = 8ull * entry_at(s + 1);
    }
};

// Segment lookup of read_elements_kernel: the list's own segment comes with the head, so near
// pointers read no table; a far pointer reads the segment count and the other segment's bounds
// from the message's table when it needs them. The head's OK status says that Message.init's
// checks passed (the table lies inside the message, and so does every segment).
struct LrSegsHead {
    const uint8_t* d;
    uint32_t known, known_off, known_len;
    uint32_t n;  // 0: not read yet
    __device__ __forceinline__ uint32_t nseg() {
        if (n == 0) n = (uint32_t)gload64(d) + 1;
        return n;
    }
    __device__ __forceinline__ uint32_t entry_at(uint32_t e) const {
        const uint64_t w = gload64(d + 4ull * (e & ~1u));
        return (e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
    }
    __device__ __forceinline__ void lookup(uint32_t s, uint64_t& off, uint64_t& slen) {
        if (s == known) {
            off = known_off;
            slen = known_len;
            return;
        }
        const uint32_t ns = nseg();
        uint64_t acc = 4ull * (1 + ns + ((ns & 1) ? 0 : 1));
        for (uint32_t i = 0; i < s; ++i) acc += 8ull * entry_at(i + 1);
        off = acc;
        slen = 8ull * entry_at(s + 1);
    }
};

// ---- resolvePointer (:451-490) ---------------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t lr_resolve(Segs& sg, LrResolved& r) {
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
__device__ __forceinline__ int32_t lr_resolve_struct(Segs& sg, uint32_t seg, uint64_t pos, uint64_t word,
                                                     LrStruct& s) {
    LrResolved r{seg, pos, word, 0, false};
    if (int32_t st = lr_resolve(sg, r)) return st;
    if (r.word == 0 || (r.word & 3) != 0) return ST_PTR;  // InvalidRootPointer
    int64_t o = (int64_t)r.pos + 8 + ptr_offset_words(r.word) * 8;
    if (r.has_over) o = (int64_t)r.over;
    if (o < 0) return ST_PTR;
    const uint32_t dw = (uint32_t)(r.word >> 32) & 0xFFFFu, pc = (uint32_t)(r.word >> 48);
    uint64_t so, sl;
    sg.lookup(r.seg, so, sl);
    if ((uint64_t)o + 8ull * (dw + pc) > sl) return ST_TRUNC;  // :514
    s = LrStruct{r.seg, so, (uint64_t)o, dw, pc};
    return ST_OK;
}

// ---- readStruct (:1224-1235) -------------------------------------------------------------------
template <class Segs>
__device__ __forceinline__ int32_t lr_step(Segs& sg, LrStruct& cur, uint32_t pi) {
    if (pi >= cur.pc) return ST_OOB;
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * pi;
    const uint64_t word = gload64(sg.d + cur.soff + ppos);
    if (word == 0) return ST_PTR;
    LrStruct next{};
    const int32_t st = lr_resolve_struct(sg, cur.seg, ppos, word, next);
    if (st == ST_OK) cur = next;
    return st;
}

// ---- resolveListPointer (:525-561) of a non-null word: the content and its byte length ---------
struct LrList {
    uint32_t seg, es;
    uint64_t soff, slen, co, cnt, bytes;
};
template <class Segs>
__device__ __forceinline__ int32_t lr_resolve_list(Segs& sg, uint32_t seg, uint64_t pos, uint64_t word,
                                                   LrList& L) {
    LrResolved r{seg, pos, word, 0, false};
    if (int32_t st = lr_resolve(sg, r)) return st;
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
    L = LrList{r.seg, es, so, sl, (uint64_t)co, cnt, bytes};
    return ST_OK;
}

// ---- one field of a struct: the data reads (:1051-1158) and the slice reads (:1187-1198, the
// typed reads, readText :1417-1443), read_fields_kernel's field body --------------------------
struct LrResult {
    int32_t st;
    uint64_t v, l, c;
};
template <class Segs>
__device__ __forceinline__ LrResult lr_read_field(Segs& sg, uint64_t moff, const LrStruct& cur,
                                                  const capnp_packed_field& F) {
    if (F.kind <= CAPNP_PACKED_FIELD_BOOL) {
        const uint32_t width = F.kind == CAPNP_PACKED_FIELD_U64 ? 8u : F.kind == CAPNP_PACKED_FIELD_U32 ? 4u
                             : F.kind == CAPNP_PACKED_FIELD_U16 ? 2u : 1u;
        if ((uint64_t)F.offset + width > 8ull * cur.dw) return LrResult{ST_OK, 0, 0, 0};
        const uint8_t* const p = sg.d + cur.soff + cur.off + (F.offset & ~7u);
        const uint32_t sh = (F.offset & 7u) * 8u;
        uint64_t v = gload64(p) >> sh;
        if ((F.offset & 7u) + width > 8u) v |= gload64(p + 8) << (64u - sh);  // sh > 0 here
        if (width < 8) v &= (1ull << (8 * width)) - 1;
        if (F.kind == CAPNP_PACKED_FIELD_BOOL) v = (v >> F.bit) & 1;
        return LrResult{ST_OK, v, width, 1};
    }
    const bool text = F.kind == CAPNP_PACKED_FIELD_TEXT;
    if (F.offset >= cur.pc) return LrResult{text ? ST_OK : ST_OOB, 0, 0, 0};
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * F.offset;
    const uint64_t word = gload64(sg.d + cur.soff + ppos);
    if (word == 0) return LrResult{text ? ST_OK : ST_PTR, 0, 0, 0};
    LrList L{};
    if (int32_t st = lr_resolve_list(sg, cur.seg, ppos, word, L)) return LrResult{st, 0, 0, 0};
    const uint32_t want = (text || F.kind == CAPNP_PACKED_FIELD_DATA) ? 2u
                        : F.kind == CAPNP_PACKED_FIELD_LIST_BIT ? 1u
                        : F.kind - CAPNP_PACKED_FIELD_LIST_16 + 3u;
    if (L.es != want) return LrResult{ST_PTR, 0, 0, 0};  // :1261 ..., InvalidTextPointer :1432
    uint64_t l = L.bytes, c = L.cnt;
    if (text && L.cnt) {  // one trailing NUL is not part of the text (:1439)
        const uint64_t last = L.co + L.cnt - 1;
        if (((gload64(sg.d + L.soff + (last & ~7ull)) >> (8 * (last & 7))) & 0xFF) == 0) {
            --l;
            --c;
        }
    }
    return LrResult{ST_OK, moff + L.soff + L.co, l, c};
}

// ---------------------------------------------------------------------------
// list_heads_kernel: Message.init, getRootStruct and readStruct along `path` as in
// read_fields_kernel, then the pointer slot `pointer_index` of that struct as
//   LIST_STRUCT   readStructList (:1165-1185) -> resolveInlineCompositeList (:563-696)
//   LIST_POINTER  readTextList / readPointerList (:1200-1222) -> resolveListPointer, element size 6
// Lane per message; one 32-byte head, a count and a status per message.
// ---------------------------------------------------------------------------
struct LrPath {
    uint32_t p[CAPNP_PACKED_MAX_PATH];
};

// the tag of an inline composite list: count, words per element (:584-596 and its two twins)
__device__ __forceinline__ int32_t lr_tag(uint64_t tag, uint32_t& count, uint32_t& dw, uint32_t& pw) {
    const int64_t c = ptr_offset_words(tag);
    if (c < 0) return ST_ICP;
    count = (uint32_t)c;
    dw = (uint32_t)(tag >> 32) & 0xFFFFu;
    pw = (uint32_t)(tag >> 48);
    return ST_OK;
}

__global__ __launch_bounds__(kBlock) void list_heads_kernel(const uint8_t* __restrict__ in,
                                                            const uint64_t* __restrict__ in_off,
                                                            const uint64_t* __restrict__ in_len, uint32_t n,
                                                            const LrPath path, uint32_t path_len,
                                                            uint32_t pointer_index, uint32_t list_kind,
                                                            capnp_packed_list_head* __restrict__ head,
                                                            uint64_t* __restrict__ count,
                                                            int32_t* __restrict__ status) {
    __shared__ uint32_t segb_all[(kSrSegs + 1) * kBlock];  // bound i of thread t at [i * kBlock + t]
    const uint32_t msg = blockIdx.x * kBlock + threadIdx.x;
    if (msg >= n) return;
    const uint64_t moff = in_off[msg];
    const uint64_t len = in_len[msg];
    const uint8_t* const d = in + moff;

    auto fail = [&](int32_t st) {
        capnp_packed_list_head h{};
        h.status = st;
        head[msg] = h;
        count[msg] = 0;
        status[msg] = st;
    };

    // ---- Message.init (:341-394), message_init_kernel's statuses ---------------------------
    if ((moff & 7) || len >= (1ull << 32)) return fail(ST_ARG);
    if (len < 4) return fail(ST_EOS);
    const uint64_t w0 = len >= 8 ? gload64(d) : (uint64_t)*reinterpret_cast<const uint32_t*>(d);
    const uint32_t m1 = (uint32_t)w0;
    if (m1 == 0xFFFFFFFFu) return fail(ST_SEGCOUNT);
    if ((uint64_t)m1 + 1 > kMsgMaxSegs) return fail(ST_SEGLIMIT);
    const uint32_t nseg = m1 + 1;
    const uint64_t header = 4ull * (1 + nseg + ((nseg & 1) ? 0 : 1));
    if (header > len) return fail(ST_TRUNC);
    uint32_t* const segb = segb_all + threadIdx.x;
    {
        uint64_t w = w0, acc = header;
        segb[0] = (uint32_t)header;
        for (uint32_t s = 0; s < nseg; ++s) {
            const uint32_t e = s + 1;
            if ((e & 1) == 0) w = gload64(d + 4ull * e);
            acc += 8ull * ((e & 1) ? (uint32_t)(w >> 32) : (uint32_t)w);
            if (acc > len) return fail(ST_TRUNC);  // :380
            if (s < kSrSegs) segb[kBlock * (s + 1)] = (uint32_t)acc;
        }
    }
    LrSegsLds sg{d, nseg, segb};

    // ---- getRootStruct (:973-985), readStruct along the path (:1224-1235) --------------------
    LrStruct cur{};
    {
        uint64_t so, sl;
        sg.lookup(0, so, sl);
        if (sl < 8) return fail(ST_TRUNC);
        if (int32_t st = lr_resolve_struct(sg, 0, 0, gload64(d + so), cur)) return fail(st);
    }
    for (uint32_t k = 0; k < path_len; ++k)
        if (int32_t st = lr_step(sg, cur, path.p[k])) return fail(st);

    // ---- the pointer slot (:1166-1172, :1188-1194) ---------------------------------------------
    if (pointer_index >= cur.pc) return fail(ST_OOB);
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * pointer_index;
    const uint64_t pword = gload64(d + cur.soff + ppos);
    if (pword == 0) return fail(ST_PTR);

    capnp_packed_list_head h{};
    if (list_kind == CAPNP_PACKED_LIST_POINTER) {
        LrList L{};
        if (int32_t st = lr_resolve_list(sg, cur.seg, ppos, pword, L)) return fail(st);
        if (L.es != 6) return fail(ST_PTR);  // :1202 / :1214
        h.elems_off = moff + L.soff + L.co;
        h.count = (uint32_t)L.cnt;
        h.segment = L.seg;
        h.seg_begin = (uint32_t)L.soff;
        h.seg_bytes = (uint32_t)L.slen;
        h.data_words = 0;
        h.pointer_words = 1;
    } else {
        // ---- resolveInlineCompositeList (:563-696): no resolvePointer, no depth ------------------
        uint32_t seg = cur.seg;
        uint64_t pos = ppos, word = pword, so = cur.soff, sl;
        {
            uint64_t o;
            sg.lookup(seg, o, sl);
        }
        uint32_t cnt = 0, dw = 0, pw = 0;
        uint64_t eo = 0;      // the elements' offset in segment `seg`
        bool resolved = false;
        if ((word & 3) == 2) {
            const bool dbl = (word >> 2) & 1;
            const uint64_t lpos = ((word >> 3) & 0x1FFFFFFFull) * 8;
            const uint32_t fseg = (uint32_t)(word >> 32);
            if (fseg >= nseg) return fail(ST_SEGID);  // :431
            uint64_t fo, fl;
            sg.lookup(fseg, fo, fl);
            if (lpos + (dbl ? 16 : 8) > fl) return fail(ST_OOB);  // :435
            const uint64_t landing = gload64(d + fo + lpos);
            if (!dbl) {
                if ((landing & 3) != 1) return fail(ST_PTR);  // :619
                seg = fseg, pos = lpos, word = landing, so = fo, sl = fl;  // the near arm at the pad
            } else {
                const uint64_t second = gload64(d + fo + lpos + 8);
                if ((landing & 3) != 2 || ((landing >> 2) & 1)) return fail(ST_FAR);  // :627/:629
                const uint32_t cseg = (uint32_t)(landing >> 32);
                if (cseg >= nseg) return fail(ST_SEGID);  // :630
                const uint64_t target = ((landing >> 3) & 0x1FFFFFFFull) * 8;
                sg.lookup(cseg, so, sl);
                seg = cseg;
                if ((second & 3) == 0) {  // layout A: the tag in the pad, bounds on count * words
                    if (int32_t st = lr_tag(second, cnt, dw, pw)) return fail(st);
                    // (:645's overflow guard cannot trip: count < 2^29, words < 2^17)
                    eo = target;
                    if (eo + 8ull * ((uint64_t)cnt * (dw + pw)) > sl) return fail(ST_OOB);  // :649
                } else if ((second & 3) == 1) {  // layout B: a list pointer in the pad, the tag at the target
                    if (((uint32_t)(second >> 32) & 7u) != 7) return fail(ST_ICP);  // :664
                    const uint64_t wc = (uint32_t)(second >> 35);
                    if (target + 8 > sl) return fail(ST_OOB);  // readWord (:668)
                    const uint64_t tag = gload64(d + so + target);
                    if ((tag & 3) != 0) return fail(ST_ICP);  // :670
                    if (int32_t st = lr_tag(tag, cnt, dw, pw)) return fail(st);
                    if ((uint64_t)cnt * (dw + pw) > wc) return fail(ST_ICP);  // :680
                    eo = target + 8;
                    if (eo + 8 * wc > sl) return fail(ST_OOB);  // :684
                } else {
                    return fail(ST_ICP);  // :695
                }
                resolved = true;
            }
        }
        if (!resolved) {
            if ((word & 3) != 1) return fail(ST_PTR);  // :611 (types 0 and 3)
            // the near arm (:572-609)
            if (((uint32_t)(word >> 32) & 7u) != 7) return fail(ST_ICP);  // :574
            const uint64_t wc = (uint32_t)(word >> 35);
            const int64_t tp = (int64_t)pos + 8 + ptr_offset_words(word) * 8;
            if (tp < 0) return fail(ST_OOB);                 // :580
            if ((uint64_t)tp + 8 > sl) return fail(ST_OOB);  // readWord (:583)
            const uint64_t tag = gload64(d + so + (uint64_t)tp);
            if ((tag & 3) != 0) return fail(ST_ICP);  // :585
            if (int32_t st = lr_tag(tag, cnt, dw, pw)) return fail(st);
            if ((uint64_t)cnt * (dw + pw) > wc) return fail(ST_ICP);  // :596
            eo = (uint64_t)tp + 8;
            if (eo + 8 * wc > sl) return fail(ST_OOB);  // :600
        }
        h.elems_off = moff + so + eo;
        h.count = cnt;
        h.segment = seg;
        h.seg_begin = (uint32_t)so;
        h.seg_bytes = (uint32_t)sl;
        h.data_words = (uint16_t)dw;
        h.pointer_words = (uint16_t)pw;
    }
    h.status = ST_OK;
    head[msg] = h;
    count[msg] = h.count;
    status[msg] = ST_OK;
}

// ---------------------------------------------------------------------------
// read_elements_kernel: lane per element, kBlock elements a block. Element e of
// [0, min(start[n], elem_cap)) belongs to the message i with start[i] <= e < start[i + 1] and is
// element k = e - start[i] of its list: StructListReader.get (list_readers.zig:87-100), or, for a
// pointer list, the pointer slot as a struct of no data words and one pointer
// (TextListReader.get :113-133, PointerListReader :243-320).
// Parent lookup: ONE wave-uniform upper_bound of `start` finds the message i0 of the block's
// first element; the block loads start[i0 .. i0 + kBlock] into LDS and each lane bisects that
// window in 8 steps. When start[i0 + kBlock] does not lie past the block's last element, more
// than kBlock messages touch this block's kBlock elements (runs of empty lists only): the block
// then falls back to a full bisection of `start` per lane, which is correct, slow and rare.
// Results are staged through LDS a group of fields at a time, as in read_fields_kernel.
// No atomics, no spins, no workspace.
// ---------------------------------------------------------------------------
// the first j in [0, n] with start[j] > e, for e < start[n]
__device__ __forceinline__ uint32_t lr_upper_bound(const uint64_t* __restrict__ start, uint32_t n, uint64_t e) {
    uint32_t lo = 0, hi = n;  // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void read_elements_kernel(const uint8_t* __restrict__ in,
                                                               const uint64_t* __restrict__ in_off, uint32_t n,
                                                               const capnp_packed_list_head* __restrict__ head,
                                                               const uint64_t* __restrict__ start,
                                                               uint32_t list_kind, uint64_t elem_cap,
                                                               const SrFields fs, uint32_t n_fields,
                                                               uint32_t* __restrict__ parent,
                                                               uint32_t* __restrict__ index,
                                                               uint64_t* __restrict__ value,
                                                               uint64_t* __restrict__ flen,
                                                               uint64_t* __restrict__ count,
                                                               int32_t* __restrict__ status) {
    __shared__ uint64_t win[kBlock + 1];                 // start[i0 + j], or ~0 past start[n]
    __shared__ uint32_t res_all[4 * kSrGroup * kBlock];  // dword i of thread t's field g at [(4 g + i) * kBlock + t]
    const uint64_t total = start[n] < elem_cap ? start[n] : elem_cap;
    const uint64_t e0 = (uint64_t)blockIdx.x * kBlock;
    if (e0 >= total) return;  // the whole block
    const uint64_t e_last = e0 + kBlock - 1 < total ? e0 + kBlock - 1 : total - 1;
    // wave-uniform: start[i0] <= e0 < start[i0 + 1] (a start array that does not begin at 0 has no
    // such i0: message 0 then, and the k check below answers). A block-cooperative search, 256
    // probes a round and 3 rounds for a million offsets, measured the same.
    const uint32_t ub0 = lr_upper_bound(start, n, e0);
    const uint32_t i0 = ub0 ? ub0 - 1 : 0;
    for (uint32_t j = threadIdx.x; j <= kBlock; j += kBlock)
        win[j] = (uint64_t)i0 + j <= n ? start[i0 + j] : ~0ull;
    __syncthreads();
    const uint64_t e = e0 + threadIdx.x;
    if (e >= total) return;
    uint32_t msg;
    uint64_t first;
    if (win[kBlock] > e_last) {  // block-uniform
        uint32_t c = 0;          // entries of win[1 .. kBlock] that are <= e: at most kBlock - 1
#pragma unroll
        for (uint32_t step = kBlock / 2; step; step >>= 1)
            if (win[c + step] <= e) c += step;
        msg = i0 + c;
        first = win[c];
    } else {
        const uint32_t ub = lr_upper_bound(start, n, e);
        msg = ub ? ub - 1 : 0;
        first = start[msg];
    }
    const uint64_t k = e - first;  // wraps far past any count when `start` is not a scan of the counts

    uint32_t* const res = res_all + threadIdx.x;
    auto store = [&](uint32_t f, int32_t st, uint64_t v, uint64_t l, uint64_t c) {
        const uint64_t at = (uint64_t)f * elem_cap + e;
        value[at] = v;
        flen[at] = l;
        if (count) count[at] = c;
        status[at] = st;
    };
    auto put = [&](uint32_t f, const LrResult& r) {
        uint32_t* const q = res + 4 * kBlock * (f % kSrGroup);
        q[0] = (uint32_t)r.v;
        q[kBlock] = (uint32_t)(r.v >> 32);
        q[2 * kBlock] = (uint32_t)r.l;
        q[3 * kBlock] = r.st == ST_OK ? (uint32_t)r.c : 0x80000000u | (uint32_t)r.st;
    };
    auto flush = [&](uint32_t f0, uint32_t f1) {  // fields [f0, f1) of one group
        for (uint32_t f = f0; f < f1; ++f) {
            const uint32_t* const q = res + 4 * kBlock * (f % kSrGroup);
            const uint32_t cs = q[3 * kBlock];
            const bool ok = !(cs >> 31);
            store(f, ok ? ST_OK : (int32_t)(cs & 0x7FFFFFFFu), (uint64_t)q[0] | ((uint64_t)q[kBlock] << 32),
                  q[2 * kBlock], ok ? cs : 0u);
        }
    };
    auto numbering = [&]() {
        if (parent) parent[e] = msg;
        if (index) index[e] = (uint32_t)k;
    };
    if (n_fields == 0) return numbering();

    const capnp_packed_list_head h = head[msg];
    if (k >= h.count) {  // `start` does not belong to these heads: nothing of the message is read
        for (uint32_t f = 0; f < n_fields; ++f) store(f, ST_ARG, 0, 0, 0);
        return numbering();
    }
    const uint64_t moff = in_off[msg];
    LrSegsHead sg{in + moff, h.segment, h.seg_begin, h.seg_bytes, 0};
    // the element (StructListReader.get's bounds check cannot fail after an OK head: the head's
    // call checked count * words, or the pointer's own word count, against the segment)
    LrStruct elem{h.segment, h.seg_begin, h.elems_off - moff - h.seg_begin, 0, 1};
    if (list_kind == CAPNP_PACKED_LIST_STRUCT) {
        elem.dw = h.data_words;
        elem.pc = h.pointer_words;
        elem.off += k * 8ull * ((uint32_t)h.data_words + h.pointer_words);
    } else {
        elem.off += 8ull * k;
    }

    LrStruct cur = elem;
    int32_t cur_st = ST_OK;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (f && f % kSrGroup == 0) flush(f - kSrGroup, f);
        const capnp_packed_field& F = fs.f[f];
        if (!((fs.same >> f) & 1)) {
            cur = elem;
            cur_st = ST_OK;
            for (uint32_t s = 0; s < F.path_len && cur_st == ST_OK; ++s) cur_st = lr_step(sg, cur, F.path[s]);
        }
        if (cur_st != ST_OK) { put(f, LrResult{cur_st, 0, 0, 0}); continue; }
        put(f, lr_read_field(sg, moff, cur, F));
    }
    flush((n_fields - 1) / kSrGroup * kSrGroup, n_fields);
    numbering();
}

}  // namespace cpk
