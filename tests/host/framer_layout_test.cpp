// The framer session's region planner (capnp-zig_amd/csrc/framer_layout.h) against a byte-array
// model of the arena and the staging buffer, on the CPU. Each plan's jobs are applied as the
// library applies them: jobs[0, first) as one launch, the others as the next, every job of a
// launch reading what was there before the launch (so a job that writes where another job of
// its launch reads or writes is a failure). After every read the model is checked in full.
// Built and run by tests/test_framer_layout.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "framer_layout.h"

namespace fl = framer_layout;

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static bool overlap(uint64_t a, uint64_t an, uint64_t b, uint64_t bn) { return an && bn && a < b + bn && b < a + an; }

static bool same(const fl::Layout& a, const fl::Layout& b) {
    return a.off == b.off && a.cap == b.cap && a.m0 == b.m0 && a.len == b.len && a.top == b.top &&
           a.moved == b.moved && a.acap == b.acap;
}

struct Model {
    uint32_t n;
    fl::Layout lay;
    std::vector<uint8_t> arena, stage;
    std::vector<std::vector<uint8_t>> held;  // per connection: the bytes fed and not popped
    std::mt19937_64 rng{0xF2A3E5};
    uint64_t reads = 0, rebuilds = 0, slides = 0, moves = 0;
    fl::Plan last;  // the plan of the last read

    explicit Model(uint32_t n_) : n(n_), held(n_) {
        for (auto* v : {&lay.off, &lay.cap, &lay.m0, &lay.len}) v->assign(n, 0);
    }

    // One launch: jobs [j0, j1) from `from` (held bytes) or the staging into `to`; in_place: they
    // are the same arena. Every job's source is read before any job writes.
    void launch(const fl::Plan& P, uint32_t j0, uint32_t j1, const std::vector<uint8_t>& from, std::vector<uint8_t>& to,
                bool in_place) {
        std::vector<std::vector<uint8_t>> bytes;
        for (uint32_t i = j0; i < j1; ++i) {
            const fl::Job& a = P.jobs[i];
            const std::vector<uint8_t>& src = a.src_kind == fl::Src::kArena ? from : stage;
            CHECK(a.len > 0, "job %u is empty", i);
            CHECK(a.dst + a.len <= P.after.acap && a.dst + a.len <= to.size(), "job %u writes past the arena", i);
            CHECK(a.src + a.len <= src.size(), "job %u reads past its source", i);
            for (uint32_t j = j0; j < j1; ++j) {
                const fl::Job& b = P.jobs[j];
                if (j != i) CHECK(!overlap(a.dst, a.len, b.dst, b.len), "jobs %u and %u of a launch write the same bytes", i, j);
                if (in_place && b.src_kind == fl::Src::kArena)
                    CHECK(!overlap(a.dst, a.len, b.src, b.len), "job %u writes what job %u of its launch reads", i, j);
            }
            bytes.emplace_back(src.begin() + a.src, src.begin() + a.src + a.len);
        }
        for (uint32_t i = j0; i < j1; ++i) std::copy(bytes[i - j0].begin(), bytes[i - j0].end(), to.begin() + P.jobs[i].dst);
    }

    // A read of add[c] new bytes per connection. fail_rebuild: the first attempt's new arena
    // "cannot be allocated": nothing may have changed, and the read is made again.
    void read(const std::vector<uint64_t>& add, bool fail_rebuild = false) {
        std::vector<uint64_t> in_off(n);
        uint64_t total = 0;
        for (uint32_t c = 0; c < n; ++c) {
            total += rng() % 3;  // gaps in the staging
            in_off[c] = total;
            total += add[c];
        }
        stage.assign(total + 8, 0);
        for (auto& b : stage) b = (uint8_t)rng();
        const fl::Layout before = lay;
        fl::Plan P = fl::plan_read(lay, in_off.data(), add.data());
        CHECK(same(lay, before), "planning changed the layout");
        if (P.rebuild && fail_rebuild) {
            const fl::Plan Q = fl::plan_read(lay, in_off.data(), add.data());  // the caller tries again
            CHECK(same(lay, before) && same(Q.after, P.after) && Q.jobs.size() == P.jobs.size() && Q.first == P.first,
                  "a failed rebuild left something behind");
        }
        CHECK(P.first <= P.jobs.size(), "first %u of %zu jobs", P.first, P.jobs.size());
        uint64_t moved = 0;
        uint32_t n_held = 0;  // slides, then moves, then appends
        for (uint32_t i = 0; i < P.jobs.size(); ++i) {
            if (P.jobs[i].src_kind != fl::Src::kArena) continue;
            CHECK(i == n_held, "job %u moves held bytes after an append", i);
            ++n_held;
            moved += P.jobs[i].len;
        }
        CHECK(P.first <= n_held, "an append among the first %u jobs", P.first);
        CHECK(P.after.moved - lay.moved == moved, "moved grew by %llu, the jobs moved %llu",
              (unsigned long long)(P.after.moved - lay.moved), (unsigned long long)moved);
        const uint32_t nj = (uint32_t)P.jobs.size();
        if (P.rebuild) {
            std::vector<uint8_t> na(P.after.acap, 0xEE);
            for (uint32_t i = P.first; i < nj; ++i) CHECK(P.jobs[i].src_kind == fl::Src::kStage, "a move after a rebuild's moves");
            launch(P, 0, P.first, arena, na, false);
            launch(P, P.first, nj, arena, na, false);
            arena.swap(na);
            ++rebuilds;
        } else {
            CHECK(P.after.acap == lay.acap, "the arena's size changed without a rebuild");
            for (uint32_t i = 0; i < P.first; ++i) {  // a slide: inside its region, to the start, source past the target
                const fl::Job& s = P.jobs[i];
                CHECK(s.dst + s.len <= s.src, "slide %u overlaps its source", i);
                bool found = false;
                for (uint32_t c = 0; c < n; ++c) found |= s.dst == lay.off[c] && s.src == lay.off[c] + lay.m0[c];
                CHECK(found, "slide %u is not a connection's held bytes to its region's start", i);
            }
            launch(P, 0, P.first, arena, arena, true);
            launch(P, P.first, nj, arena, arena, true);
            slides += P.first;
            moves += n_held - P.first;
        }
        for (uint32_t c = 0; c < n; ++c)
            held[c].insert(held[c].end(), stage.begin() + in_off[c], stage.begin() + in_off[c] + add[c]);
        lay = P.after;
        last = std::move(P);
        ++reads;
        check();
    }

    void pop(uint32_t c, uint64_t bytes) {  // whole messages left the connection
        CHECK(bytes <= held[c].size(), "test: pop past the held bytes");
        lay.m0[c] += bytes;
        held[c].erase(held[c].begin(), held[c].begin() + bytes);
    }
    void reset(uint32_t c) {
        lay.m0[c] = lay.len[c] = 0;
        held[c].clear();
    }

    void check() const {
        CHECK(lay.top <= lay.acap && lay.acap <= arena.size(), "top %llu acap %llu", (unsigned long long)lay.top,
              (unsigned long long)lay.acap);
        for (uint32_t c = 0; c < n; ++c) {
            CHECK(lay.m0[c] <= lay.len[c] && lay.len[c] <= lay.cap[c], "connection %u: m0 %llu len %llu cap %llu", c,
                  (unsigned long long)lay.m0[c], (unsigned long long)lay.len[c], (unsigned long long)lay.cap[c]);
            CHECK(lay.off[c] + lay.cap[c] <= lay.top, "connection %u: region past the arena top", c);
            CHECK(lay.len[c] - lay.m0[c] == held[c].size(), "connection %u holds %llu bytes, fed minus popped is %zu", c,
                  (unsigned long long)(lay.len[c] - lay.m0[c]), held[c].size());
            CHECK(std::equal(held[c].begin(), held[c].end(), arena.begin() + lay.off[c] + lay.m0[c]),
                  "connection %u: its bytes in the arena are not the bytes fed", c);
            for (uint32_t d = 0; d < c; ++d)
                CHECK(!overlap(lay.off[c], lay.cap[c], lay.off[d], lay.cap[d]), "regions of %u and %u overlap", d, c);
        }
    }

    std::vector<uint64_t> only(uint32_t c, uint64_t bytes) const {
        std::vector<uint64_t> add(n, 0);
        add[c] = bytes;
        return add;
    }
};

// Connection c with an empty region of exactly 64 KiB, the others holding a few bytes.
static Model fresh(uint32_t n, uint32_t c) {
    Model m(n);
    std::vector<uint64_t> add(n, 3);
    add[c] = 1;
    m.read(add);
    m.reset(c);
    CHECK(m.lay.cap[c] == 65536 && m.lay.len[c] == 0, "test: no fresh 64-KiB region");
    return m;
}

static void edges(uint32_t n) {
    const uint32_t c = n - 1;
    {   // no bytes at all: nothing to do
        Model m = fresh(n, c);
        const fl::Layout before = m.lay;
        m.read(std::vector<uint64_t>(n, 0));
        CHECK(m.last.jobs.empty() && !m.last.rebuild && same(m.lay, before), "an empty read planned something");
    }
    for (uint64_t bytes : {1ull, 65535ull, 65536ull, 65537ull}) {  // around the fresh region's size
        Model m = fresh(n, c);
        const uint64_t off = m.lay.off[c];
        m.read(m.only(c, bytes), true);
        if (bytes <= 65536)
            CHECK(m.last.jobs.size() == 1 && !m.last.rebuild && m.lay.off[c] == off && m.lay.cap[c] == 65536,
                  "%llu bytes did not go into the fresh region", (unsigned long long)bytes);
        else
            CHECK(m.lay.cap[c] == fl::region_for(bytes) && (m.last.rebuild || m.lay.off[c] != off),
                  "%llu bytes did not get a new region", (unsigned long long)bytes);
    }
    for (uint64_t extra : {0ull, 1ull}) {  // a held tail of m0 (slides) and of m0 + 1 bytes (does not)
        Model m = fresh(n, c);
        const uint64_t off = m.lay.off[c], m0 = 32768 - extra;
        m.read(m.only(c, 2 * m0 + extra));
        m.pop(c, m0);
        CHECK(m.lay.m0[c] == m0 && m.lay.len[c] - m0 == m0 + extra && m.lay.off[c] == off, "test: tail not set up");
        m.read(m.only(c, 100 + 2 * extra), true);  // passes the region's end, would fit after a slide
        if (!extra)
            CHECK(m.last.first == 1 && !m.last.rebuild && m.lay.off[c] == off && m.lay.m0[c] == 0, "a tail of m0 bytes did not slide");
        else
            CHECK((m.last.rebuild || m.last.first == 0) && (m.last.rebuild || m.lay.off[c] != off),
                  "a tail of m0 + 1 bytes slid onto itself");
    }
    {   // drained to m0 == len: restarts at its region's start, nothing moves
        Model m = fresh(n, c);
        const uint64_t off = m.lay.off[c], moved = m.lay.moved;
        m.read(m.only(c, 60000));
        m.pop(c, 60000);
        m.read(m.only(c, 10000));
        CHECK(m.last.jobs.size() == 1 && m.lay.off[c] == off && m.lay.m0[c] == 0 && m.lay.len[c] == 10000 &&
                  m.lay.moved == moved, "a drained connection did not restart at its region's start");
    }
    for (uint64_t extra : {0ull, 1ull}) {  // a new region that fills the arena top exactly, and one byte more
        Model m = fresh(n, c);
        m.read(m.only(c, 1));
        const uint64_t room = m.lay.acap - m.lay.top, acap = m.lay.acap;
        CHECK(room % 512 == 0 && room / 2 > 65536, "test: the arena's free top is %llu", (unsigned long long)room);
        m.read(m.only(c, room / 2 - 1 + extra), true);  // want = room / 2 (+ 1): a region of room bytes (+ 256)
        if (!extra)
            CHECK(!m.last.rebuild && m.lay.acap == acap && m.lay.top == acap, "filling the top exactly rebuilt the arena");
        else
            CHECK(m.last.rebuild && m.lay.acap > acap, "a region one step past the top did not rebuild the arena");
    }
}

// Reads of mixed sizes with pops and resets in between, for about a second.
static void walk(uint32_t n, uint32_t reads, uint64_t seed, Model& sum) {
    Model m(n);
    std::mt19937_64 rng(seed);
    for (uint32_t r = 0; r < reads; ++r) {
        std::vector<uint64_t> add(n, 0);
        for (uint32_t c = 0; c < n; ++c) {
            switch (rng() % 8) {
                case 0: break;
                case 1: add[c] = 1 + rng() % 16; break;
                case 2: add[c] = 65530 + rng() % 12; break;
                case 3: add[c] = rng() % 5 ? 0 : 100000 + rng() % 200000; break;
                default: add[c] = rng() % 6000; break;
            }
        }
        m.read(add, rng() % 2);
        for (uint32_t c = 0; c < n; ++c) {
            const uint64_t have = m.held[c].size();
            switch (rng() % 6) {
                case 0: break;
                case 1: m.pop(c, have); break;
                case 2: if (rng() % 8 == 0) m.reset(c); break;
                default: m.pop(c, have ? rng() % (have + 1) : 0); break;
            }
        }
    }
    sum.reads += m.reads;
    sum.rebuilds += m.rebuilds;
    sum.slides += m.slides;
    sum.moves += m.moves;
}

int main() {
    Model sum(1);
    for (uint32_t n : {1u, 2u, 5u}) {
        edges(n);
        walk(n, 1200, 0x5EED0000 + n, sum);
    }
    CHECK(sum.rebuilds > 3 && sum.slides > 10 && sum.moves > 10, "the walk took %llu rebuilds, %llu slides, %llu moves",
          (unsigned long long)sum.rebuilds, (unsigned long long)sum.slides, (unsigned long long)sum.moves);
    std::printf("framer_layout ok: %llu reads, %llu arena rebuilds, %llu slides, %llu moves to the arena top\n",
                (unsigned long long)sum.reads, (unsigned long long)sum.rebuilds, (unsigned long long)sum.slides,
                (unsigned long long)sum.moves);
    return 0;
}
