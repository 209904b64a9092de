// kernels/list_read.h
// Struct lists and pointer lists of decoded messages as element tables:
// list_heads_kernel (one list per message: readStructList / readTextList / readPointerList, lane
// per message) and read_elements_kernel (fields of every element of every list as columns, lane
// per element). Both walk the message with message_walk.h's functions, as read_fields_kernel does.
// Leans on:
//   common.h             kBlock, the ST_* statuses, capnp_packed_field / _list_head
//   device_helpers.h     gload64, ptr_offset_words
//   message_walk.h       mw_init, MwSegsLds, mw_root, mw_step, mw_resolve_list, mw_read_fields, mw_entry_at,
//                        MwStage, SrFields, kSrSegs, kSrGroup
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"
#include "kernels/device_helpers.h"
#include "kernels/message_walk.h"

namespace cpk {

// Segment lookup of read_elements_kernel: the list's own segment comes with the head, so near
// pointers read no table; a far pointer reads the segment count and the other segment's bounds
// from the message's table when it needs them. The head's OK status says that Message.init's
// checks passed (the table lies inside the message, and so does every segment).
struct MwSegsHead {
    const uint8_t* d;
    uint32_t known, known_off, known_len;
    uint32_t n;  // 0: not read yet
    __device__ __forceinline__ uint32_t nseg() {
        if (n == 0) n = (uint32_t)gload64(d) + 1;
        return n;
    }
    __device__ __forceinline__ void lookup(uint32_t s, uint64_t& off, uint64_t& slen) {
        if (s == known) {
            off = known_off;
            slen = known_len;
            return;
        }
        const uint32_t ns = nseg();
        uint64_t acc = 4ull * (1 + ns + ((ns & 1) ? 0 : 1));
        for (uint32_t i = 0; i < s; ++i) acc += 8ull * mw_entry_at(d, i + 1);
        off = acc;
        slen = 8ull * mw_entry_at(d, s + 1);
    }
};

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

    // ---- Message.init, getRootStruct, readStruct along the path (:1224-1235) -------------------
    uint32_t nseg;
    if (int32_t st = mw_init(d, moff, len, segb_all + threadIdx.x, nseg)) return fail(st);
    MwSegsLds sg{d, nseg, segb_all + threadIdx.x};
    MwStruct cur{};
    if (int32_t st = mw_root(sg, cur)) return fail(st);
    for (uint32_t k = 0; k < path_len; ++k)
        if (int32_t st = mw_step(sg, cur, path.p[k])) return fail(st);

    // ---- the pointer slot (:1166-1172, :1188-1194) ---------------------------------------------
    if (pointer_index >= cur.pc) return fail(ST_OOB);
    const uint64_t ppos = cur.off + 8ull * cur.dw + 8ull * pointer_index;
    const uint64_t pword = gload64(d + cur.soff + ppos);
    if (pword == 0) return fail(ST_PTR);

    capnp_packed_list_head h{};
    if (list_kind == CAPNP_PACKED_LIST_POINTER) {
        MwList L{};
        if (int32_t st = mw_resolve_list(sg, cur.seg, ppos, pword, L)) return fail(st);
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
// Results are staged through LDS a group of fields at a time (MwStage), as in read_fields_kernel.
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

    const MwStage out{res_all + threadIdx.x, e, elem_cap, value, flen, count, status};
    auto numbering = [&]() {
        if (parent) parent[e] = msg;
        if (index) index[e] = (uint32_t)k;
    };
    if (n_fields == 0) return numbering();

    const capnp_packed_list_head h = head[msg];
    if (k >= h.count) {  // `start` does not belong to these heads: nothing of the message is read
        out.store_all(n_fields, ST_ARG);
        return numbering();
    }
    const uint64_t moff = in_off[msg];
    MwSegsHead sg{in + moff, h.segment, h.seg_begin, h.seg_bytes, 0};
    // the element (StructListReader.get's bounds check cannot fail after an OK head: the head's
    // call checked count * words, or the pointer's own word count, against the segment)
    MwStruct elem{h.segment, h.seg_begin, h.elems_off - moff - h.seg_begin, 0, 1};
    if (list_kind == CAPNP_PACKED_LIST_STRUCT) {
        elem.dw = h.data_words;
        elem.pc = h.pointer_words;
        elem.off += k * 8ull * ((uint32_t)h.data_words + h.pointer_words);
    } else {
        elem.off += 8ull * k;
    }

    mw_read_fields(sg, moff, elem, fs, n_fields, out);
    numbering();
}

}  // namespace cpk
