// build_plan.h
// The static half of capnp_packed_build_fields_batch: the plan the host
// compiles from the caller's ops (sb_compile, which is also the call's host-side check) and the
// per-message layout function (sb_layout: the checks of the table in capnp_packed.h and the
// start word of every op's allocation). No HIP dependency: the C-ABI layer, the kernel
// (kernels/struct_build.h) and a plain host program (tests/host_build/) compile the same text.
//
// The reference's allocation rule (message.zig:1701-1707, :1799, :1870, :1936-1940, :2085-2092):
// every call appends to the end of segment 0, in call order. Word 0 of the segment is the root
// pointer, then op 0's struct, then each later op's allocation: a struct's data_words +
// pointer_words (none for (0, 0): writeStructPointer :1851-1860 writes a null pointer), a
// slice's content padded to the word (Text: its bytes and a NUL), nothing for an absent op.
#pragma once
#include <stdint.h>

#include "capnp_packed.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CPK_SB_HD __host__ __device__ inline
#else
#define CPK_SB_HD inline
#endif

namespace cpk {

constexpr uint32_t kSbMaxOps = CAPNP_PACKED_MAX_BUILD_OPS;
constexpr uint32_t kSbMaxWords = CAPNP_PACKED_MAX_BUILD_WORDS;  // the root pointer + every struct word
constexpr uint32_t kSbNoOp = 0xFFu;

// what an op does in the kernel
enum : uint8_t {
    SB_NONE = 0,    // a data write that does not lie wholly inside the data section: dropped
    SB_DATA = 1,    // writeU8/16/32/64: `width` bytes at byte `shift` of plan word `word`
    SB_BOOL = 2,    // writeBool: bit `width` of byte `shift` of plan word `word`
    SB_SLICE = 3,   // writeText / writeData / write*List: a ragged allocation
    SB_STRUCT = 4,  // allocateStruct / initStruct: `swords` words
};

struct SbOp {
    uint8_t what;    // SB_*
    uint8_t kind;    // the caller's CAPNP_PACKED_FIELD_* (SB_SLICE)
    uint8_t shift;   // SB_DATA / SB_BOOL: byte in the first word, 0-7
    uint8_t width;   // SB_DATA: 1, 2, 4, 8; SB_BOOL: the bit
    uint16_t word;   // SB_DATA / SB_BOOL: plan word of the write's first byte
    uint16_t swords; // SB_STRUCT: data_words + pointer_words
    uint16_t dw, pw; // SB_STRUCT
    uint16_t pad;
};

// One computed word of a message. Plan word 0 is the root pointer; the words of the structs
// follow in op order (their place in the message depends on the slices in between).
struct SbWord {
    uint8_t owner;   // the SB_STRUCT op whose struct holds the word (plan word 0: 0, not used)
    uint8_t local;   // its index in that struct
    uint8_t ptr_op;  // a pointer word: the op that fills it, or kSbNoOp (null); data words: kSbNoOp
    uint8_t is_ptr;
};

struct SbPlan {
    uint32_t n_ops;
    uint32_t n_words;  // 1 + the words of every struct, at most kSbMaxWords
    uint32_t has_bits; // some op is LIST_BIT: the count column is read
    uint32_t pad;
    SbOp op[kSbMaxOps];
    SbWord word[kSbMaxWords];
};

CPK_SB_HD bool sb_is_slice(uint32_t kind) {
    return kind >= CAPNP_PACKED_FIELD_TEXT && kind <= CAPNP_PACKED_FIELD_LIST_64;
}
CPK_SB_HD bool sb_is_data(uint32_t kind) { return kind <= CAPNP_PACKED_FIELD_BOOL; }

// The plan of `ops`, or the reason it is refused (every host-side check of the call that
// concerns the ops). Returns nullptr when the plan stands.
inline const char* sb_compile(const capnp_packed_build_op* ops, uint32_t n_ops, SbPlan* plan) {
    *plan = SbPlan{};
    if (n_ops > kSbMaxOps) return "more than 32 build ops";
    if (n_ops == 0) return "no build ops";
    if (!ops) return "null ops";
    if (ops[0].kind != CAPNP_PACKED_BUILD_STRUCT) return "op 0 is not BUILD_STRUCT";
    uint16_t base[kSbMaxOps] = {};  // plan word of a struct op's first word
    uint32_t words = 1;             // the root pointer
    plan->n_ops = n_ops;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const capnp_packed_build_op& a = ops[k];
        SbOp& o = plan->op[k];
        const bool is_struct = a.kind == CAPNP_PACKED_BUILD_STRUCT;
        if (!is_struct && a.kind > CAPNP_PACKED_FIELD_LIST_64) return "unknown build op kind";
        if (a.bit > (a.kind == CAPNP_PACKED_FIELD_BOOL ? 7u : 0u)) return "bit is 0-7 for BOOL and 0 otherwise";
        if (a.reserved[0] | a.reserved[1] | a.reserved[2]) return "reserved is not 0";
        if (k > 0) {
            if (a.target >= k || ops[a.target].kind != CAPNP_PACKED_BUILD_STRUCT)
                return "target is not an earlier BUILD_STRUCT op";
        }
        const capnp_packed_build_op& t = ops[k ? a.target : 0];
        if (k > 0 && (is_struct || sb_is_slice(a.kind))) {  // fills a pointer slot of its target
            if (a.offset >= t.pointer_words) return "pointer index past the target's pointer section";
            SbWord& w = plan->word[base[a.target] + t.data_words + a.offset];
            if (w.ptr_op != kSbNoOp) return "two ops on one pointer slot";
            w.ptr_op = (uint8_t)k;
        }
        if (is_struct) {
            const uint32_t sw = (uint32_t)a.data_words + a.pointer_words;
            if (words + sw > kSbMaxWords) return "more than 64 struct words with the root pointer";
            o.what = SB_STRUCT;
            o.swords = (uint16_t)sw;
            o.dw = a.data_words;
            o.pw = a.pointer_words;
            base[k] = (uint16_t)words;
            for (uint32_t i = 0; i < sw; ++i)
                plan->word[words + i] = SbWord{(uint8_t)k, (uint8_t)i, (uint8_t)kSbNoOp, (uint8_t)(i >= a.data_words)};
            words += sw;
        } else if (sb_is_slice(a.kind)) {
            o.what = SB_SLICE;
            o.kind = (uint8_t)a.kind;
            if (a.kind == CAPNP_PACKED_FIELD_LIST_BIT) plan->has_bits = 1;
        } else {
            // struct_builder.zig:356-458: a write that does not lie wholly inside the data
            // section is dropped
            const uint32_t width = a.kind == CAPNP_PACKED_FIELD_BOOL ? 1u : 1u << a.kind;
            const uint64_t data_bytes = 8ull * t.data_words;
            if ((uint64_t)a.offset + width > data_bytes) {
                o.what = SB_NONE;
            } else {
                o.what = a.kind == CAPNP_PACKED_FIELD_BOOL ? SB_BOOL : SB_DATA;
                o.word = (uint16_t)(base[k ? a.target : 0] + a.offset / 8);
                o.shift = (uint8_t)(a.offset % 8);
                o.width = a.kind == CAPNP_PACKED_FIELD_BOOL ? (uint8_t)a.bit : (uint8_t)width;
            }
        }
    }
    plan->word[0] = SbWord{0, 0, 0, 1};  // the root pointer: op 0's struct
    plan->n_words = words;
    return nullptr;
}

// A present slice's bytes before padding (Text: with its NUL; message.zig:1799) and the words
// its allocation takes (:1796-1804, :1934-1940). The one place these rules stand: sb_slice,
// sb_layout and the kernel's passes all call them.
CPK_SB_HD uint64_t sb_slice_bytes(uint32_t kind, uint64_t len) {
    return len + (kind == CAPNP_PACKED_FIELD_TEXT ? 1u : 0u);  // len < 2^64 - 1: ABSENT is not a length
}
CPK_SB_HD uint64_t sb_slice_words(uint32_t kind, uint64_t len) { return (sb_slice_bytes(kind, len) + 7) >> 3; }
// the element count of its list pointer (Text: with the NUL, :1812; a bit list: the count column)
CPK_SB_HD uint64_t sb_slice_elems(uint32_t kind, uint64_t len, uint64_t count) {
    switch (kind) {
        case CAPNP_PACKED_FIELD_LIST_BIT: return count;
        case CAPNP_PACKED_FIELD_LIST_16:
        case CAPNP_PACKED_FIELD_LIST_32:
        case CAPNP_PACKED_FIELD_LIST_64: return len >> (kind - CAPNP_PACKED_FIELD_LIST_16 + 1);
        default: return sb_slice_bytes(kind, len);  // TEXT, DATA
    }
}

// One slice op of one message: its checks in the order of capnp_packed.h's table (status 0 =
// passes). `len` is not CAPNP_PACKED_BUILD_ABSENT.
CPK_SB_HD int32_t sb_slice(uint32_t kind, uint64_t off, uint64_t len, uint64_t count, uint64_t pool_len) {
    if (kind == CAPNP_PACKED_FIELD_LIST_BIT) {
        if (count > UINT64_MAX - 7 || len != (count + 7) / 8) return CAPNP_PACKED_INVALID_ARGUMENT;
    } else if (kind >= CAPNP_PACKED_FIELD_LIST_16) {
        if (len & ((2ull << (kind - CAPNP_PACKED_FIELD_LIST_16)) - 1)) return CAPNP_PACKED_INVALID_ARGUMENT;
    }
    if (sb_slice_elems(kind, len, count) >= (1ull << 29)) return CAPNP_PACKED_LIST_TOO_LARGE;
    if (off > pool_len || len > pool_len - off) return CAPNP_PACKED_OUT_OF_BOUNDS;
    return CAPNP_PACKED_OK;
}

// the element size code of a slice kind's list pointer (message.zig:37-43, :65-76)
CPK_SB_HD uint32_t sb_elem_size(uint32_t kind) {
    switch (kind) {
        case CAPNP_PACKED_FIELD_LIST_BIT: return 1;
        case CAPNP_PACKED_FIELD_LIST_16: return 3;
        case CAPNP_PACKED_FIELD_LIST_32: return 4;
        case CAPNP_PACKED_FIELD_LIST_64: return 5;
        default: return 2;  // TEXT, DATA
    }
}

// The layout of one message. `col` gives op k's column entries: col.value(k), col.len(k),
// col.count(k) (count is asked of LIST_BIT ops only). Runs the slice checks in op order; on
// success *seg_words is the length of segment 0 in words (the framed message has one more, the
// segment table) and, where `start` is not null, start[k] is the segment word at which op k's
// allocation begins (for an op that allocates nothing: where the next one will).
template <class Col>
CPK_SB_HD int32_t sb_layout(const SbPlan& p, const Col& col, uint64_t pool_len, uint64_t* seg_words, uint64_t* start) {
    uint64_t cur = 1;  // the root pointer
    for (uint32_t k = 0; k < p.n_ops; ++k) {
        const SbOp& o = p.op[k];
        if (start) start[k] = cur;
        if (o.what == SB_STRUCT) {
            cur += o.swords;
        } else if (o.what == SB_SLICE) {
            const uint64_t len = col.len(k);
            if (len == CAPNP_PACKED_BUILD_ABSENT) continue;
            const int32_t st = sb_slice(o.kind, col.value(k), len,
                                        o.kind == CAPNP_PACKED_FIELD_LIST_BIT ? col.count(k) : 0, pool_len);
            if (st) return st;
            cur += sb_slice_words(o.kind, len);
        }
    }
    *seg_words = cur;
    return CAPNP_PACKED_OK;
}

}  // namespace cpk
