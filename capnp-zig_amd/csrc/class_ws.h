// class_ws.h — the class workspace `q` of a batch of n units, as plain arithmetic: no HIP and no
// device pointers, but for q_tiles (the reserved counter's accessor, which the tile, window and
// splitter kernels share; compiled under hipcc only). Every batch encode, decode and decoded-size call classes its units into this
// block (class_count / class_scan / class_scatter_kernel, packed_kernels.hip) and every later
// kernel of the call reads it; the framer's spec block (capnp_packed_abi.cpp: SpecBlock) is the
// head and the window table of the same layout. tests/host/class_ws_test.cpp pins every
// number below on the CPU.
//
// The workspace is an array of u32, queue_bytes(n) = class_ws_bytes(n) bytes, in this order
// (u32 indices unless bytes are named):
//
//   head             [0, kQHead): counters and cursors, cleared and set by the class pass
//       kSlotLong        long units listed
//       kSlotHuge        huge units listed (more than kQHuge packed / plain bytes)
//       kSlotSmall       small units listed
//       kSlotMid         mid units listed (all bins)
//       kSlotSerial      units on the serial list
//       kSlotReserved    tiles (encode) / windows (decode, framer) reserved: a u64, two slots
//       kSlotSerialTake  encode_tiled_kernel's take cursor into the serial list
//       kSlotMidBefore+b mid units in the bins before bin b, b < CL_MID_BINS
//       kSlotTwoPass     decode: the mid list's [0, this) is the two-pass decoder's share, the
//                        rest the words decoder's
//       kSlotCapped      decode: words-decoder units stopped at their slot's capacity
//       slots 1, 6, 7, 19 and 22 .. 31 are unused (zeroed with the rest of the head)
//   long / huge list [long_list_off(), + n): long units from the front upwards, huge units from
//                    the back downwards; walked huge units first (long_list_slot). The long
//                    window pass overwrites an entry with the unit's first window.
//   small list       [small_list_off(n), + n)
//   mid list         [mid_list_off(n), + n): the bins in order
//   block counts     [block_counts_off(n), + kClassK * class_blocks(n)): per class block, the
//                    units per class, then (scanned) the exclusive prefixes over blocks
//   serial list      [serial_off(n), + n): long units the tile / window table could not hold
//   tile table       encode, 8-byte aligned, tile_cap(n) entries of kTileEntBytes in columns:
//                    sizes (u64) at tile_tab_off(n), units at tile_unit_off(n), first tiles at
//                    tile_first_off(n)
//   window table     decode and framer, 16-byte aligned, IN THE SAME SPACE as the tile table (a
//                    call uses one of the two): win_cap(n) entries of kWinEntBytes at
//                    win_tab_off(n)
//   record region    bytes, 256-byte aligned, after the longer of the two tables: kRecStride
//                    bytes of piece records per mid-list entry at rec_region_off(n)
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CPK_HD __host__ __device__
#else
#define CPK_HD
#endif

namespace cpk {

constexpr uint32_t kQHead = 32;         // u32 slots of the head
constexpr uint32_t kClassBlock = 1024;  // units per class-kernel block
constexpr uint32_t kClassK = 12;        // per-block class counters (11 classes used)
constexpr uint32_t CL_MID_BINS = 8;     // bins of the mid list (classes CL_MID + 0 .. 7)
constexpr uint64_t kTileExtra = 65536;  // tile table: capacity n + kTileExtra tiles
constexpr uint64_t kWinExtra = 32768;   // window table: capacity n / 8 + kWinExtra windows
constexpr uint64_t kTileEntBytes = 16;  // a tile's size (u64), unit and first tile (u32 each)
constexpr uint64_t kWinEntBytes = 176;  // sizeof(WinEnt)
constexpr uint64_t kRecBytes = 704;     // kRecStride

constexpr uint32_t kSlotLong = 0;
constexpr uint32_t kSlotHuge = 2;
constexpr uint32_t kSlotSmall = 3;
constexpr uint32_t kSlotMid = 4;
constexpr uint32_t kSlotSerial = 5;
constexpr uint32_t kSlotReserved = 8;  // and 9: a u64
constexpr uint32_t kSlotSerialTake = 10;
constexpr uint32_t kSlotMidBefore = 11;  // .. 11 + CL_MID_BINS - 1
constexpr uint32_t kSlotTwoPass = 20;
constexpr uint32_t kSlotCapped = 21;

// every named slot once, inside the head
constexpr bool head_slots_distinct() {
    bool used[kQHead] = {};
    const uint32_t single[] = {kSlotLong,     kSlotHuge,         kSlotSmall,      kSlotMid,     kSlotSerial,
                               kSlotReserved, kSlotReserved + 1, kSlotSerialTake, kSlotTwoPass, kSlotCapped};
    for (uint32_t s : single) {
        if (s >= kQHead || used[s]) return false;
        used[s] = true;
    }
    for (uint32_t b = 0; b < CL_MID_BINS; ++b) {
        if (kSlotMidBefore + b >= kQHead || used[kSlotMidBefore + b]) return false;
        used[kSlotMidBefore + b] = true;
    }
    return true;
}
static_assert(head_slots_distinct(), "head slots overlap or leave the head");
static_assert(kSlotReserved % 2 == 0, "the u64 counter is 8-byte aligned");
static_assert(kSlotMidBefore + CL_MID_BINS <= kSlotTwoPass, "the bin prefixes end before slot 20");
static_assert(kSlotCapped < kQHead && kSlotTwoPass < kQHead, "slots lie in the head");

// The slot holding the count of mid units up to and including bin b: the next bin's prefix, or
// the mid total.
CPK_HD constexpr uint32_t mid_through_slot(uint32_t b) { return b + 1 < CL_MID_BINS ? kSlotMidBefore + b + 1 : kSlotMid; }

CPK_HD inline uint64_t class_blocks(uint64_t n) { return (n + kClassBlock - 1) / kClassBlock; }

// ---- regions (u32 indices) ----
CPK_HD constexpr uint32_t long_list_off() { return kQHead; }
CPK_HD inline uint64_t small_list_off(uint64_t n) { return kQHead + n; }
CPK_HD inline uint64_t mid_list_off(uint64_t n) { return kQHead + 2 * n; }
CPK_HD inline uint64_t block_counts_off(uint64_t n) { return kQHead + 3 * n; }
CPK_HD inline uint64_t serial_off(uint64_t n) { return kQHead + 3 * n + kClassK * class_blocks(n); }
CPK_HD inline uint64_t tile_cap(uint64_t n) { return n + kTileExtra; }
CPK_HD inline uint64_t tile_tab_off(uint64_t n) { return (serial_off(n) + n + 1) & ~1ull; }  // 8-B aligned
// the units column of a table of cap tiles, from the table's start: after cap sizes (u64)
CPK_HD inline uint64_t tile_unit_col(uint64_t cap) { return 2 * cap; }
CPK_HD inline uint64_t tile_unit_off(uint64_t n) { return tile_tab_off(n) + tile_unit_col(tile_cap(n)); }
CPK_HD inline uint64_t tile_first_off(uint64_t n) { return tile_unit_off(n) + tile_cap(n); }
CPK_HD inline uint64_t win_cap(uint64_t n) { return n / 8 + kWinExtra; }
CPK_HD inline uint64_t win_tab_off(uint64_t n) { return (tile_tab_off(n) + 3) & ~3ull; }  // 16-B aligned

// ---- regions (bytes) ----
CPK_HD inline uint64_t tile_tab_end_bytes(uint64_t n) { return tile_tab_off(n) * sizeof(uint32_t) + kTileEntBytes * tile_cap(n); }
CPK_HD inline uint64_t win_tab_bytes_off(uint64_t n) { return win_tab_off(n) * sizeof(uint32_t); }
CPK_HD inline uint64_t win_tab_end_bytes(uint64_t n) { return win_tab_bytes_off(n) + kWinEntBytes * win_cap(n); }
CPK_HD inline uint64_t rec_region_off(uint64_t n) {
    const uint64_t tiles = tile_tab_end_bytes(n), wins = win_tab_end_bytes(n);
    return ((tiles > wins ? tiles : wins) + 255) & ~255ull;
}
CPK_HD inline uint64_t class_ws_bytes(uint64_t n) { return rec_region_off(n) + kRecBytes * n; }
// The framer's spec block for nl listed connections and `windows` windows in all: a head and a
// window table placed as in a workspace of nl units, holding exactly the windows.
CPK_HD inline uint64_t framer_spec_ws_bytes(uint64_t nl, uint64_t windows) {
    return win_tab_bytes_off(nl) + kWinEntBytes * windows;
}

// ---- the long / huge list ----
// Slot of the idx-th long unit (upwards) and of the idx-th huge unit (downwards), in u32 as the
// kernels index: n + kQHead must not pass 2^32 (such a workspace is terabytes; no batch has one).
CPK_HD inline uint32_t long_slot(uint32_t idx) { return kQHead + idx; }
CPK_HD inline uint32_t huge_slot(uint32_t n, uint32_t idx) { return kQHead + n - 1 - idx; }
// The walk of the list's nh huge and nl long units, huge units first: entry i < nh + nl.
CPK_HD inline uint32_t long_list_slot(uint32_t n, uint32_t nh, uint32_t i) {
    return i < nh ? huge_slot(n, i) : long_slot(i - nh);
}

// ---- device accessors (HIP only) ----
#ifdef __HIPCC__
// tiles / windows reserved so far (u64)
__device__ __forceinline__ unsigned long long* q_tiles(uint32_t* q) {
    return reinterpret_cast<unsigned long long*>(q + kSlotReserved);
}
#endif

// What a launcher passes to kernels that take a list or a counter instead of the workspace.
struct ClassWs {
    uint32_t* q;
    uint32_t n;
    uint32_t* slot(uint32_t s) const { return q + s; }
    const uint32_t* mid() const { return q + mid_list_off(n); }
    const uint32_t* serial() const { return q + serial_off(n); }
    uint8_t* rec() const { return reinterpret_cast<uint8_t*>(q) + rec_region_off(n); }
};

}  // namespace cpk
