// tests/host_build/build_host.cpp
// build_plan.h on the host: the plan compiler (sb_compile) and the per-message layout function
// (sb_layout) that capnp_packed_build_fields_batch's kernel runs per lane.
//   build_host_main N             N generated programs (valid and invalid) with generated
//                                 lengths; asserts the invariants below; exit status 0 = all held
//   build_host_main IN OUT        the cases of text file IN (tests/test_host_build.py writes it
//                                 from the model's corpus); per message "status seg_words
//                                 start[0..n_ops)" to OUT, or "refused" for a refused program
// Invariants: every plan entry lies inside CAPNP_PACKED_MAX_BUILD_WORDS; a pointer word names an
// op that fills a pointer slot; allocations are disjoint and in op order (start[k + 1] >= start[k],
// a struct's words and a present slice's padded bytes between them); the total is their sum + the
// root pointer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "build_plan.h"

using namespace cpk;

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

struct Cols {
    const uint64_t* v;  // per op: value, len, count
    uint64_t value(uint32_t k) const { return v[3 * k]; }
    uint64_t len(uint32_t k) const { return v[3 * k + 1]; }
    uint64_t count(uint32_t k) const { return v[3 * k + 2]; }
};

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static void check_plan(const capnp_packed_build_op* ops, uint32_t n_ops, const SbPlan& p) {
    REQUIRE(p.n_ops == n_ops && p.n_words >= 1 && p.n_words <= kSbMaxWords);
    uint32_t words = 1;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const SbOp& o = p.op[k];
        REQUIRE(o.what <= SB_STRUCT);
        if (o.what == SB_STRUCT) {
            REQUIRE(o.swords == o.dw + o.pw && o.dw == ops[k].data_words && o.pw == ops[k].pointer_words);
            for (uint32_t i = 0; i < o.swords; ++i) {
                const SbWord& w = p.word[words + i];
                REQUIRE(w.owner == k && w.local == i && w.is_ptr == (i >= o.dw));
                if (w.ptr_op != kSbNoOp) {
                    REQUIRE(w.is_ptr && w.ptr_op > k && w.ptr_op < n_ops);
                    REQUIRE(p.op[w.ptr_op].what == SB_STRUCT || p.op[w.ptr_op].what == SB_SLICE);
                    REQUIRE(ops[w.ptr_op].target == k && ops[w.ptr_op].offset == i - o.dw);
                }
            }
            words += o.swords;
        } else if (o.what == SB_DATA || o.what == SB_BOOL) {
            const uint32_t bytes = o.what == SB_BOOL ? 1u : o.width;
            REQUIRE(o.shift < 8 && o.word >= 1 && o.word < p.n_words);
            const uint32_t last = o.word + (o.shift + bytes - 1) / 8;  // the word of the write's last byte
            REQUIRE(last < p.n_words);
            const SbWord &a = p.word[o.word], &b = p.word[last];
            REQUIRE(!a.is_ptr && !b.is_ptr && a.owner == ops[k].target && b.owner == a.owner);
        }
    }
    REQUIRE(words == p.n_words);
}

static void check_layout(const SbPlan& p, const uint64_t* cols, uint64_t pool_len) {
    uint64_t start[kSbMaxOps + 1], total = 0;
    const int32_t st = sb_layout(p, Cols{cols}, pool_len, &total, start);
    if (st) {
        REQUIRE(st == CAPNP_PACKED_INVALID_ARGUMENT || st == CAPNP_PACKED_LIST_TOO_LARGE ||
                st == CAPNP_PACKED_OUT_OF_BOUNDS);
        return;
    }
    uint64_t cur = 1;
    for (uint32_t k = 0; k < p.n_ops; ++k) {
        REQUIRE(start[k] == cur);  // in op order, no gap and no overlap
        const SbOp& o = p.op[k];
        if (o.what == SB_STRUCT) cur += o.swords;
        if (o.what == SB_SLICE && cols[3 * k + 1] != CAPNP_PACKED_BUILD_ABSENT) {
            // restated here on purpose, not through sb_slice_words: Text's NUL, then whole words
            const uint64_t bytes = cols[3 * k + 1] + (o.kind == CAPNP_PACKED_FIELD_TEXT ? 1 : 0);
            REQUIRE(bytes <= (1ull << 32));
            REQUIRE(sb_slice_words(o.kind, cols[3 * k + 1]) == (bytes + 7) / 8);
            REQUIRE(sb_slice_elems(o.kind, cols[3 * k + 1], cols[3 * k + 2]) < (1ull << 29));
            cur += (bytes + 7) / 8;
        }
    }
    REQUIRE(total == cur);
}

static int fuzz(long cases) {
    long accepted = 0;
    for (long c = 0; c < cases; ++c) {
        capnp_packed_build_op ops[kSbMaxOps + 2];
        memset(ops, 0, sizeof ops);
        const uint32_t n_ops = below(kSbMaxOps + 2);
        const bool wild = below(4) == 0;  // often invalid: any target, index, kind
        for (uint32_t k = 0; k < n_ops; ++k) {
            capnp_packed_build_op& a = ops[k];
            const uint32_t r = below(16);
            a.kind = (k == 0 || r < 3) ? CAPNP_PACKED_BUILD_STRUCT : (wild && r == 15 ? 11 + below(8) : below(11));
            a.target = k ? (wild ? below(k + 2) : below(k)) : below(3);
            if (!wild && k && ops[a.target].kind != CAPNP_PACKED_BUILD_STRUCT) a.target = 0;
            a.offset = below(wild ? 80 : 12);
            a.bit = a.kind == CAPNP_PACKED_FIELD_BOOL ? below(wild ? 10 : 8) : (wild && below(8) == 0);
            if (a.kind == CAPNP_PACKED_BUILD_STRUCT) {
                a.data_words = (uint16_t)below(wild ? 40 : 4);
                a.pointer_words = (uint16_t)below(wild ? 40 : 6);
            }
            if (wild && below(40) == 0) a.reserved[below(3)] = 1;
        }
        SbPlan plan;
        if (sb_compile(ops, n_ops, &plan)) continue;
        ++accepted;
        check_plan(ops, n_ops, plan);
        for (int row = 0; row < 4; ++row) {
            uint64_t cols[3 * kSbMaxOps];
            const uint64_t pool_len = below(3) ? 1ull << below(40) : below(5000);
            for (uint32_t k = 0; k < n_ops; ++k) {
                const uint32_t r = below(16);
                uint64_t len = r == 0 ? CAPNP_PACKED_BUILD_ABSENT : r == 1 ? rnd() : r == 2 ? rnd() >> below(64) : below(5000);
                if (ops[k].kind >= CAPNP_PACKED_FIELD_LIST_16 && r > 3) len &= ~((2ull << (ops[k].kind - CAPNP_PACKED_FIELD_LIST_16)) - 1);
                uint64_t count = r == 4 ? rnd() : len * 8 - (len && len != CAPNP_PACKED_BUILD_ABSENT ? below(8) : 0);
                cols[3 * k] = r == 5 ? rnd() : below(6000);
                cols[3 * k + 1] = len;
                cols[3 * k + 2] = count;
            }
            check_layout(plan, cols, pool_len);
        }
    }
    printf("build_host: %ld programs, %ld accepted, every invariant held\n", cases, accepted);
    return accepted ? 0 : 1;
}

static int replay(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "r");
    FILE* out = fopen(out_path, "w");
    REQUIRE(in && out);
    uint32_t n_ops;
    uint64_t pool_len;
    while (fscanf(in, "%u %" SCNu64, &n_ops, &pool_len) == 2) {
        REQUIRE(n_ops <= 64);
        std::vector<capnp_packed_build_op> ops(n_ops ? n_ops : 1);
        memset(ops.data(), 0, ops.size() * sizeof ops[0]);
        for (uint32_t k = 0; k < n_ops; ++k) {
            unsigned dw, pw;
            REQUIRE(fscanf(in, "%u %u %u %u %u %u %u", &ops[k].kind, &ops[k].target, &ops[k].offset, &ops[k].bit, &dw,
                           &pw, &ops[k].reserved[2]) == 7);
            ops[k].data_words = (uint16_t)dw;
            ops[k].pointer_words = (uint16_t)pw;
        }
        uint32_t rows;
        REQUIRE(fscanf(in, "%u", &rows) == 1);
        SbPlan plan;
        const char* why = sb_compile(ops.data(), n_ops, &plan);
        if (!why) check_plan(ops.data(), n_ops, plan);
        fprintf(out, why ? "refused\n" : "accepted %u\n", plan.n_words);
        for (uint32_t r = 0; r < rows; ++r) {
            std::vector<uint64_t> cols(3 * (n_ops ? n_ops : 1));
            for (uint32_t k = 0; k < 3 * n_ops; ++k) REQUIRE(fscanf(in, "%" SCNu64, &cols[k]) == 1);
            if (why) continue;
            uint64_t start[kSbMaxOps], total = 0;
            const int32_t st = sb_layout(plan, Cols{cols.data()}, pool_len, &total, start);
            fprintf(out, "%d %" PRIu64, st, st ? 0 : total);
            for (uint32_t k = 0; !st && k < n_ops; ++k) fprintf(out, " %" PRIu64, start[k]);
            fprintf(out, "\n");
        }
    }
    fclose(in);
    fclose(out);
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(capnp_packed_build_op) == 32, "capnp_packed_build_op is 32 bytes");
    if (argc == 3) return replay(argv[1], argv[2]);
    return fuzz(argc == 2 ? atol(argv[1]) : 20000);
}
