// The class workspace layout (capnp-zig_amd/csrc/class_ws.h) on the CPU. Includes only that
// header. Every region offset is compared with the formula written out again here in literals,
// the regions are checked for order, overlap, alignment and 64-bit wrap, long_list_slot is
// enumerated, and the total and the framer's spec size are compared with a table recorded from
// capnp_packed_batch_workspace_bytes / cpk::framer_spec_bytes of the build before the layout
// was named (pure host arithmetic, called on a machine without a GPU).
#include "class_ws.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int g_fail = 0;
#define CHECK(c, n)                                                                           \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            std::printf("FAIL line %d, n = %llu: %s\n", __LINE__, (unsigned long long)(n), #c); \
            ++g_fail;                                                                         \
        }                                                                                     \
    } while (0)

struct Total {
    uint32_t n;
    uint64_t bytes;
};
const Total kTotals[] = {
    {1u, 5768128ull},           {2u, 5768832ull},          {7u, 5772608ull},
    {8u, 5773312ull},           {9u, 5774016ull},          {1023u, 6526272ull},
    {1024u, 6527232ull},        {1025u, 6527936ull},       {65535u, 54397248ull},
    {65536u, 54398208ull},      {1048575u, 783859008ull},  {1048576u, 783859968ull},
    {1048577u, 783860672ull},   {16777216u, 12455248128ull}, {4294967295u, 3187072826688ull},
};
struct Spec {
    uint32_t nl;
    uint64_t windows, bytes;
};
const Spec kSpecs[] = {{1u, 1ull, 368ull}, {7u, 100ull, 17888ull}, {1025u, 4096ull, 737520ull}};

void check_regions(uint64_t n, uint64_t recorded_total) {
    using namespace cpk;
    // the formulas again, in literals
    const uint64_t lists = 32;
    const uint64_t blocks = (n + 1023) / 1024;
    const uint64_t serial = 32 + 3 * n + 12 * blocks;
    const uint64_t tile = (serial + n + 1) & ~1ull;
    const uint64_t tcap = n + 65536;
    const uint64_t win = (tile + 3) & ~3ull;
    const uint64_t wcap = n / 8 + 32768;
    const uint64_t tile_end = 4 * tile + 16 * tcap, win_end = 4 * win + 176 * wcap;
    const uint64_t rec = ((tile_end > win_end ? tile_end : win_end) + 255) & ~255ull;
    const uint64_t total = rec + 704 * n;

    CHECK(kQHead == 32 && kClassBlock == 1024 && kClassK == 12 && CL_MID_BINS == 8, n);
    CHECK(kTileExtra == 65536 && kWinExtra == 32768, n);
    CHECK(kTileEntBytes == 16 && kWinEntBytes == 176 && kRecBytes == 704, n);
    CHECK(long_list_off() == lists, n);
    CHECK(small_list_off(n) == 32 + n, n);
    CHECK(mid_list_off(n) == 32 + 2 * n, n);
    CHECK(block_counts_off(n) == 32 + 3 * n, n);
    CHECK(class_blocks(n) == blocks, n);
    CHECK(serial_off(n) == serial, n);
    CHECK(tile_tab_off(n) == tile, n);
    CHECK(tile_cap(n) == tcap, n);
    CHECK(tile_unit_off(n) == tile + 2 * tcap, n);
    CHECK(tile_first_off(n) == tile + 3 * tcap, n);
    CHECK(tile_tab_end_bytes(n) == tile_end, n);
    CHECK(win_tab_off(n) == win, n);
    CHECK(win_tab_bytes_off(n) == 4 * win, n);
    CHECK(win_cap(n) == wcap, n);
    CHECK(win_tab_end_bytes(n) == win_end, n);
    CHECK(rec_region_off(n) == rec, n);
    CHECK(class_ws_bytes(n) == total, n);
    CHECK(class_ws_bytes(n) == recorded_total, n);

    // order and no overlap: each region starts at or after the end of the one before (u32
    // indices up to the tables, bytes from there); the two tables share their space
    CHECK(kQHead <= long_list_off(), n);
    CHECK(long_list_off() + n <= small_list_off(n), n);
    CHECK(small_list_off(n) + n <= mid_list_off(n), n);
    CHECK(mid_list_off(n) + n <= block_counts_off(n), n);
    CHECK(block_counts_off(n) + kClassK * class_blocks(n) <= serial_off(n), n);
    CHECK(serial_off(n) + n <= tile_tab_off(n), n);
    CHECK(serial_off(n) + n <= win_tab_off(n), n);
    CHECK(tile_tab_off(n) < tile_unit_off(n) && tile_unit_off(n) < tile_first_off(n), n);
    CHECK(tile_unit_off(n) - tile_tab_off(n) == 2 * tile_cap(n), n);  // cap sizes of 8 bytes
    CHECK(4 * (tile_first_off(n) + tile_cap(n)) == tile_tab_end_bytes(n), n);
    CHECK(tile_tab_end_bytes(n) <= rec_region_off(n), n);
    CHECK(win_tab_end_bytes(n) <= rec_region_off(n), n);
    CHECK(rec_region_off(n) + kRecBytes * n == class_ws_bytes(n), n);
    // alignment
    CHECK(4 * tile_tab_off(n) % 8 == 0, n);
    CHECK(win_tab_bytes_off(n) % 16 == 0, n);
    CHECK(rec_region_off(n) % 256 == 0, n);
    // nothing wrapped: the total again in 128 bits (every offset before it is at most the total)
    typedef unsigned __int128 u128;
    const u128 serial_w = 32 + (u128)3 * n + (u128)12 * blocks, tile_w = (serial_w + n + 1) & ~(u128)1;
    const u128 tile_end_w = 4 * tile_w + (u128)16 * tcap, win_end_w = 4 * ((tile_w + 3) & ~(u128)3) + (u128)176 * wcap;
    const u128 total_w = (((tile_end_w > win_end_w ? tile_end_w : win_end_w) + 255) & ~(u128)255) + (u128)704 * n;
    CHECK(total_w == (u128)class_ws_bytes(n) && total_w < ((u128)1 << 63), n);
}

// long_list_slot over entries [0, nh + nl) names every slot of [kQHead, kQHead + n) once. The
// accessor works in u32, as the kernels index: n + kQHead must stay below 2^32.
void check_long_list(uint32_t n, uint32_t nh) {
    using namespace cpk;
    std::vector<uint8_t> seen(n, 0);
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = long_list_slot(n, nh, i);
        if (s < kQHead || s - kQHead >= n || seen[s - kQHead]++) ++bad;
    }
    CHECK(bad == 0, n);
    if (nh) CHECK(long_list_slot(n, nh, 0) == huge_slot(n, 0) && huge_slot(n, 0) == 32 + n - 1, n);  // huge first, from the back
    if (nh < n) CHECK(long_list_slot(n, nh, nh) == long_slot(0) && long_slot(0) == 32, n);
}

}  // namespace

int main() {
    for (const Total& t : kTotals) {
        check_regions(t.n, t.bytes);
        if (t.n <= 9) {
            for (uint32_t nh = 0; nh <= t.n; ++nh) check_long_list(t.n, nh);
        } else if (t.n <= (1u << 24)) {
            check_long_list(t.n, 0);
            check_long_list(t.n, t.n);
            check_long_list(t.n, 1);
        } else {
            // n = 0xFFFFFFFF: no u32 slot index reaches its list's end (kQHead + n passes 2^32), in
            // the header as in the kernels before it; such a workspace is 3 TB and is never
            // allocated. The walk's ends are checked at the largest n a u32 index serves.
            const uint32_t m = 0xFFFFFFFFu - cpk::kQHead;
            for (uint32_t nh : {0u, m, 1u}) {
                if (nh) CHECK(cpk::long_list_slot(m, nh, 0) == 0xFFFFFFFEu, m);          // the list's last slot
                if (nh) CHECK(cpk::long_list_slot(m, nh, nh - 1) == 32 + (m - nh), m);   // the huge part's lowest
                if (nh < m) CHECK(cpk::long_list_slot(m, nh, nh) == 32, m);              // the long part's first
                if (nh < m) CHECK(cpk::long_list_slot(m, nh, m - 1) == 32 + (m - nh) - 1, m);  // and last, just below
            }
        }
    }
    for (const Spec& s : kSpecs) {
        CHECK(cpk::framer_spec_ws_bytes(s.nl, s.windows) == s.bytes, s.nl);
        CHECK(cpk::framer_spec_ws_bytes(s.nl, s.windows) == 4 * cpk::win_tab_off(s.nl) + 176 * s.windows, s.nl);
    }
    // the head: the slots by number
    using namespace cpk;
    CHECK(kSlotLong == 0 && kSlotHuge == 2 && kSlotSmall == 3 && kSlotMid == 4 && kSlotSerial == 5, 0);
    CHECK(kSlotReserved == 8 && kSlotSerialTake == 10 && kSlotMidBefore == 11 && kSlotTwoPass == 20 && kSlotCapped == 21, 0);
    for (uint32_t b = 0; b < CL_MID_BINS; ++b) CHECK(mid_through_slot(b) == (b < 7 ? 12 + b : 4), b);
    if (g_fail) return 1;
    std::printf("class_ws ok\n");
    return 0;
}
