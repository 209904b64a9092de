// framer_layout.h — where a framer session's bytes live, as plain arithmetic:
// no HIP, no device pointers. capnp_packed_abi.cpp carries a plan out;
// tests/host/framer_layout_test.cpp runs plans against a byte-array model on the CPU.
//
// Regions: a connection's region is [off, off + cap) of the arena, its bytes [m0, len) of
// it. A read that does not fit moves the connection's bytes to a fresh region of twice their
// size at the arena top (the bytes of a partial message move once per doubling); when the
// top reaches the end, every connection's bytes move to a new arena of twice the live size.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace framer_layout {

inline uint64_t region_for(uint64_t bytes) { return std::max<uint64_t>(65536, (2 * bytes + 255) & ~255ull); }

struct Layout {
    std::vector<uint64_t> off, cap, m0, len;  // per connection
    uint64_t top = 0;    // the arena below `top` is given to regions
    uint64_t moved = 0;  // bytes moved between regions so far
    uint64_t acap = 0;   // the arena's size
};

// One copy of a read. The target is always the arena the plan leaves current (the new one
// after a rebuild), so the source is never the new arena: held bytes come from the arena
// before the read, new bytes from the staging buffer.
enum class Src : uint8_t { kArena, kStage };
struct Job {
    uint64_t dst;  // offset in the arena after the read
    Src src_kind;
    uint64_t src;  // offset in the arena before the read, or in the staging
    uint64_t len;
};

// A read's region layout and the copies that make it true. The caller commits `after` only
// once every copy is enqueued: a failed allocation or launch leaves the session as it was.
// jobs[0, first) run before the others, which may overwrite their source:
// - rebuild: the moves into a new arena of after.acap bytes, run to completion from the
//   current arena (which stays valid), then the appends;
// - else: the slides, as a launch of their own, then the moves to the top and the appends.
struct Plan {
    Layout after;
    bool rebuild = false;
    std::vector<Job> jobs;
    uint32_t first = 0;
};

// A connection whose bytes would pass its region's end slides its held bytes to the region's
// start when they and the new bytes fit there and the slide's source and target do not overlap
// (held <= m0; a drained connection just restarts there); else it gets a new region.
inline bool slides(const Layout& L, uint32_t c, uint64_t add) {
    const uint64_t held = L.len[c] - L.m0[c];
    return add && L.len[c] + add > L.cap[c] && held + add <= L.cap[c] && held <= L.m0[c];
}

// The plan of a read that brings in_len[c] new bytes per connection, found at in_off[c] of the
// staging buffer.
inline Plan plan_read(const Layout& cur, const uint64_t* in_off, const uint64_t* in_len) {
    const uint32_t n = (uint32_t)cur.off.size();
    std::vector<uint64_t> want(n, 0);  // a connection's bytes after this read
    uint64_t grow_bytes = 0;
    bool any_grow = false;
    for (uint32_t c = 0; c < n; ++c) {
        want[c] = cur.len[c] - cur.m0[c] + in_len[c];
        if (in_len[c] && cur.len[c] + in_len[c] > cur.cap[c] && !slides(cur, c, in_len[c])) {
            any_grow = true;
            grow_bytes += region_for(want[c]);
        }
    }
    Plan P;
    P.after = cur;
    Layout& L = P.after;
    auto move_to = [&](uint32_t c, uint64_t at, uint64_t rc) {  // c's held bytes to a region [at, at + rc)
        const uint64_t held = L.len[c] - L.m0[c];
        if (held) {
            P.jobs.push_back({at, Src::kArena, L.off[c] + L.m0[c], held});
            L.moved += held;
        }
        L.off[c] = at;
        L.cap[c] = rc;
        L.m0[c] = 0;
        L.len[c] = held;
    };
    if (any_grow && cur.top + grow_bytes > cur.acap) {
        // a new arena, every region sized for its bytes after this read
        P.rebuild = true;
        uint64_t t = 0;
        for (uint32_t c = 0; c < n; ++c) {
            if (!want[c]) {
                L.off[c] = L.cap[c] = L.m0[c] = L.len[c] = 0;
                continue;
            }
            const uint64_t rc = region_for(want[c]);
            move_to(c, t, rc);
            t += rc;
        }
        L.top = t;
        L.acap = std::max<uint64_t>(2 * t, 1u << 20);
        P.first = (uint32_t)P.jobs.size();
    } else {
        for (uint32_t c = 0; c < n; ++c)
            if (slides(cur, c, in_len[c])) move_to(c, L.off[c], L.cap[c]);
        P.first = (uint32_t)P.jobs.size();
        for (uint32_t c = 0; any_grow && c < n; ++c) {  // the slid ones fit now
            if (!in_len[c] || L.len[c] + in_len[c] <= L.cap[c]) continue;
            const uint64_t rc = region_for(want[c]);
            move_to(c, L.top, rc);
            L.top += rc;
        }
    }
    for (uint32_t c = 0; c < n; ++c) {
        if (!in_len[c]) continue;
        P.jobs.push_back({L.off[c] + L.len[c], Src::kStage, in_off[c], in_len[c]});
        L.len[c] += in_len[c];
    }
    return P;
}

}  // namespace framer_layout
