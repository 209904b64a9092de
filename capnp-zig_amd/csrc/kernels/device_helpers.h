// kernels/device_helpers.h
// The small device helpers every path shares: global / LDS loads, DPP wave scans, wave_reserve
// (a shared counter's ranges, one atomic per wave), the compact / expand selectors and their LUTs,
// partial 16-B stores, vmcnt_at_most. DESIGN.md §2.2 (scans, selectors), §2.3 (ring loads), §2.6
// (wave_reserve).
// Leans on:
//   common.h             kWave
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/common.h"

namespace cpk {

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 16 readable bytes for load lanes that have nothing to stage, and 16 writable
// bytes for the piece-record stores of lanes without a unit.
__device__ __attribute__((aligned(16))) uint8_t cpk_dummy16[16];
__device__ __attribute__((aligned(16))) uint8_t cpk_sink16[16];
__device__ __attribute__((aligned(64))) uint8_t cpk_sink64[64];

// 16-B load of data read for the last time (non-temporal). The fill pass's piece loads
// use it (decode 2.42 -> 2.40 ms); encode's staging loads were slower with it.
__device__ __forceinline__ uint4 load_nt(const void* p) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

// Ring loads of the lane-per-unit
// decoders in inline asm, so hipcc neither turns them into FLAT instructions
// (pointers that went through __shfl / LDS lose their address space, and FLAT counts on
// lgkmcnt too: every LDS wait of the walk would wait for the prefetch) nor waits for them
// itself (its own vmcnt(0) before the ring writes would also wait for the previous round's
// stores). The kernels count them (s_waitcnt vmcnt(N)) and pin the loaded registers after
// the wait (cdna_hip_programming.md §5.7 item 1, form ii).
__device__ __forceinline__ void ds_gload16(u32x4& d, const void* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}

// LDS-DMA: each lane's 16 B at gsrc straight into LDS at lds_base + 16 * lane (no VGPR
// destination; count it with vmcnt, then a barrier before other waves read it). M0 is written
// and restored in the same statement (cdna_hip_programming.md §5.7).
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_base) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_base) : "memory");
}
// the LDS byte address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) uint8_t*)p);
}

// Order LDS traffic between lanes of ONE wave (the wave owns its LDS slice).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// a 64-bit value from lane `src` (two 32-bit shuffles, zero-extended halves: an int | u64 would
// sign-extend the low half)
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}


// Wave scans on DPP: row_shr:1/2/4/8 inside each 16-lane row, then row_bcast:15 and
// row_bcast:31 across rows (gfx9). A lane a step does not reach keeps `ident`. No LDS
// round trips (the ds_bpermute scans they replace cost ~6 LDS latencies in a row).
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v, uint32_t ident) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)ident, (int)v, CTRL, ROWS, 0xF, false);
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
    v += dpp_mov<0x111, 0xF>(v, 0u);
    v += dpp_mov<0x112, 0xF>(v, 0u);
    v += dpp_mov<0x114, 0xF>(v, 0u);
    v += dpp_mov<0x118, 0xF>(v, 0u);
    v += dpp_mov<0x142, 0xA>(v, 0u);
    v += dpp_mov<0x143, 0xC>(v, 0u);
    return v;
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
    v = max(v, dpp_mov<0x111, 0xF>(v, 0u));
    v = max(v, dpp_mov<0x112, 0xF>(v, 0u));
    v = max(v, dpp_mov<0x114, 0xF>(v, 0u));
    v = max(v, dpp_mov<0x118, 0xF>(v, 0u));
    v = max(v, dpp_mov<0x142, 0xA>(v, 0u));
    v = max(v, dpp_mov<0x143, 0xC>(v, 0u));
    return v;
}

__device__ __forceinline__ uint32_t wave_incl_min(uint32_t v) {
    v = min(v, dpp_mov<0x111, 0xF>(v, ~0u));
    v = min(v, dpp_mov<0x112, 0xF>(v, ~0u));
    v = min(v, dpp_mov<0x114, 0xF>(v, ~0u));
    v = min(v, dpp_mov<0x118, 0xF>(v, ~0u));
    v = min(v, dpp_mov<0x142, 0xA>(v, ~0u));
    v = min(v, dpp_mov<0x143, 0xC>(v, ~0u));
    return v;
}

// the wave's minimum / maximum, wave-uniform (the scan's last lane)
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    return __builtin_amdgcn_readlane(wave_incl_min(v), kWave - 1);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    return __builtin_amdgcn_readlane(wave_incl_max(v), kWave - 1);
}

// The DPP scan of a u64 sum, in place: per step moves on both halves and a 64-bit add. A macro,
// so both functions below get the statements themselves (through a helper function, inlined,
// the compiler split the adds and the kernels' code changed).
#define CPK_SUM64_STEP(V, CTRL, ROWS)                                                           \
    V += (uint64_t)dpp_mov<CTRL, ROWS>((uint32_t)V, 0u) | ((uint64_t)dpp_mov<CTRL, ROWS>((uint32_t)(V >> 32), 0u) << 32)
#define CPK_SUM64_SCAN(V)          \
    CPK_SUM64_STEP(V, 0x111, 0xF); \
    CPK_SUM64_STEP(V, 0x112, 0xF); \
    CPK_SUM64_STEP(V, 0x114, 0xF); \
    CPK_SUM64_STEP(V, 0x118, 0xF); \
    CPK_SUM64_STEP(V, 0x142, 0xA); \
    CPK_SUM64_STEP(V, 0x143, 0xC)
// inclusive sum of a u64 over the wave
__device__ __forceinline__ uint64_t wave_incl_sum64(uint64_t v) {
    CPK_SUM64_SCAN(v);
    return v;
}
// sum of a u64 over the wave, wave-uniform
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    CPK_SUM64_SCAN(v);
    return (uint64_t)__builtin_amdgcn_readlane((uint32_t)v, kWave - 1) |
           ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), kWave - 1) << 32);
}
#undef CPK_SUM64_SCAN
#undef CPK_SUM64_STEP

// the previous lane's v (wave_shr:1); lane 0 gets ident
__device__ __forceinline__ uint32_t wave_prev_lane(uint32_t v, uint32_t ident) { return dpp_mov<0x138, 0xF>(v, ident); }

// Lane l - 1's v (lane 0: 0), read with every lane active: the asm pins the DPP move (and
// the computation of v) in front of any branch on the lane, since a DPP read of a lane the
// EXEC mask excludes returns that lane's stale register.
__device__ __forceinline__ uint32_t fu_prev_lane(uint32_t v) {
    uint32_t r = dpp_mov<0x138, 0xF>(v, 0u);
    asm volatile("" : "+v"(r));
    return r;
}

// v of the first lane above this one with `has` set, or `none` (encode_tile's run ends)
__device__ __forceinline__ uint32_t next_break(bool has, uint32_t v, uint32_t lane, uint32_t none) {
    const uint64_t above = (__builtin_amdgcn_ballot_w64(has) >> lane) >> 1;  // lanes > this one
    const uint32_t src = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : lane;
    const uint32_t r = (uint32_t)__shfl((int)v, (int)src, kWave);
    return above ? r : none;
}

__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t l) {
    return __builtin_amdgcn_readlane(v, l);
}

// Consecutive ranges of a shared counter for a wave's lanes (k each, 0: none), in lane order,
// with ONE atomic per wave: ~10K long units each adding to the one counter serialised at its L2
// channel while the small-unit kernel loaded the memory system (config C5: 0.21 ms).
__device__ __forceinline__ uint64_t wave_reserve(unsigned long long* ctr, uint64_t k) {
    const uint32_t lane = lane_id();
    uint64_t incl = k;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t o = __shfl_up(incl, d, kWave);
        if (lane >= (uint32_t)d) incl += o;
    }
    const uint64_t total = __shfl(incl, kWave - 1, kWave);
    uint64_t b = 0;
    if (lane == 0 && total != 0) b = atomicAdd(ctr, (unsigned long long)total);
    b = __shfl(b, 0, kWave);
    return b + incl - k;
}

// Zero-byte tag of a little-endian word: bit k set <=> byte k != 0
// (message.zig:257-262 builds the same tag byte-by-byte).
__device__ __forceinline__ uint32_t nonzero_tag(uint64_t w) {
    // byte k of c: bit 0 = byte k nonzero, bit 4 = byte k + 4 nonzero; the dot product with
    // 2^k gathers them (one full-rate v_dot4 instead of two quarter-rate multiplies)
    const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
    const uint32_t yl = ((lo & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | lo, yh = ((hi & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | hi;
    const uint32_t c = ((yl >> 7) & 0x01010101u) | ((yh >> 3) & 0x10101010u);
    return __builtin_amdgcn_udot4(c, 0x08040201u, 0u, false);
}

// v_perm_b32 over the 8 bytes of d: selector byte r in 0..7 picks byte r, 0x0C gives 0.
__device__ __forceinline__ uint64_t perm64(uint64_t d, uint64_t sel) {
    uint32_t lo = (uint32_t)d, hi = (uint32_t)(d >> 32);
    uint32_t a = __builtin_amdgcn_perm(hi, lo, (uint32_t)sel);
    uint32_t b = __builtin_amdgcn_perm(hi, lo, (uint32_t)(sel >> 32));
    return (uint64_t)a | ((uint64_t)b << 32);
}

// v_perm_b32 selector tables, built at compile time (a block copies one into LDS):
//   compact: gathers the nonzero bytes of a word with tag t into bytes 0..popc-1
//            (0x0C = zero above them);
//   expand:  scatters popc(t) packed bytes back to the set-bit positions of t.
struct alignas(16) SelLut {
    uint64_t v[256];
};
constexpr SelLut make_sel_lut(bool expand) {
    SelLut lut{};
    for (uint32_t t = 0; t < 256; ++t) {
        uint64_t sel = expand ? 0ull : 0x0C0C0C0C0C0C0C0CULL;
        uint32_t r = 0;
        for (uint32_t k = 0; k < 8; ++k) {
            const bool set = (t >> k) & 1u;
            if (expand) {
                sel |= (set ? (uint64_t)(r++) : 0x0Cull) << (8 * k);
            } else if (set) {
                sel = (sel & ~(0xFFULL << (8 * r))) | ((uint64_t)k << (8 * r));
                ++r;
            }
        }
        lut.v[t] = sel;
    }
    return lut;
}
__device__ constexpr SelLut kCompactLut = make_sel_lut(false);
__device__ constexpr SelLut kExpandLut = make_sel_lut(true);
// The compact selector moved up one byte (byte 0 selects a zero byte): perm64(w, it) is the
// tag's record payload at bytes 1..popc, ready to OR with the tag (encode_tile).
__device__ __forceinline__ uint64_t compact_selector(uint32_t t) { return (kCompactLut.v[t] << 8) | 0x0Cull; }
// the same as a table, for a copy into LDS by LDS-DMA (encode_kernel)
constexpr SelLut make_compact_sel() {
    SelLut l = make_sel_lut(false);
    for (uint32_t t = 0; t < 256; ++t) l.v[t] = (l.v[t] << 8) | 0x0Cull;
    return l;
}
__device__ constexpr SelLut kCompactSel = make_compact_sel();
__device__ __forceinline__ uint64_t expand_selector(uint32_t t) { return kExpandLut.v[t]; }

// Unaligned 8-byte read from an LDS byte array as two aligned ds_read_b64 and a branch-free
// funnel shift (a byte-aligned ds_read_b64 is legal on gfx950 but measured ~2x slower in the
// expand loop: the LDS splits it).
__device__ __forceinline__ uint64_t lds_u64_at(const uint8_t* base, uint32_t p) {
    const uint32_t a = p & ~7u;
    const uint64_t lo = *reinterpret_cast<const uint64_t*>(base + a);
    const uint64_t hi = *reinterpret_cast<const uint64_t*>(base + a + 8);
    const uint32_t s = (p & 7u) * 8u;
    return (lo >> s) | ((hi << 1) << (63u - s));
}

// 8-byte global loads: gload64 where p is known 8-aligned, ld_u64 / ld_u32 at any alignment
// (gfx950 unaligned access: still one global_load_dwordx2 / dword).
__device__ __forceinline__ uint64_t gload64(const uint8_t* p) {
    return *reinterpret_cast<const uint64_t*>(p);
}
__device__ __forceinline__ uint64_t ld_u64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// a struct / list pointer's signed 30-bit offset in words (Message.validate, the struct reads)
__device__ __forceinline__ int64_t ptr_offset_words(uint64_t w) {  // message.zig:11-18
    const uint32_t raw = (uint32_t)((w >> 2) & 0x3FFFFFFFu);
    return (raw & 0x20000000u) ? (int64_t)raw - ((int64_t)1 << 30) : (int64_t)raw;
}

// Stage nch 16-B chunks from global g[0 .. 16*nch) into lds[0 .. 16*nch):
// lane l moves chunks l, l+64, ... Loads AND stores are unconditional, with the
// chunk index clamped to nch-1 (a clamped lane re-writes the last chunk with the
// same bytes), so the compiler cannot sink the loads into guarded blocks: all K
// loads are in flight together and one vmcnt wait lands them.
template <int K>
__device__ __forceinline__ void stage_linear(uint8_t* lds, const uint8_t* g, uint32_t nch, uint32_t lane) {
    if (nch == 0) return;
    uint4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = min(lane + 64u * k, nch - 1);
        v[k] = *reinterpret_cast<const uint4*>(g + 16 * (uint64_t)c);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = min(lane + 64u * k, nch - 1);
        *reinterpret_cast<uint4*>(lds + 16 * c) = v[k];
    }
}

// Bytes [lo, hi) (0 <= lo < hi <= 16) of a 16-B chunk (x0 = bytes 0-7, x1 = bytes 8-15)
// whose 16-B aligned home is c16: naturally aligned 1/2/4/8-B stores, up to 8-B alignment
// and then down from it (at most 8 predicated stores). A byte loop runs to the wave's
// longest partial chunk (C5 small encode: ~100 us of 400).
__device__ __forceinline__ void store_partial16(uint8_t* c16, uint32_t lo, uint32_t hi, uint64_t x0, uint64_t x1) {
    auto put = [&](uint32_t sz) {  // bytes [lo, lo + sz), lo aligned to sz
        const uint64_t v = lo < 8 ? x0 >> (8 * lo) : x1 >> (8 * (lo - 8));
        uint8_t* const p = c16 + lo;
        if (sz == 8) *reinterpret_cast<uint64_t*>(p) = v;
        else if (sz == 4) *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
        else if (sz == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
        else *p = (uint8_t)v;
        lo += sz;
    };
    if ((lo & 1) && lo + 1 <= hi) put(1);
    if ((lo & 2) && lo + 2 <= hi) put(2);
    if ((lo & 4) && lo + 4 <= hi) put(4);
    if (lo + 8 <= hi) put(8);
    if (lo + 4 <= hi) put(4);
    if (lo + 2 <= hi) put(2);
    if (lo + 1 <= hi) put(1);
}
// The same through global (address space 1) pointers, for kernels that count their LDS waits:
// a generic pointer would make FLAT stores, which also count on lgkmcnt. (One template over the
// pointer type changed the code of the kernels that use either, so both stay.)
__device__ __forceinline__ void es_store_partial16(uint8_t* c16, uint32_t lo, uint32_t hi, uint64_t x0, uint64_t x1) {
    typedef __attribute__((address_space(1))) uint8_t g8;
    typedef __attribute__((address_space(1))) uint16_t g16;
    typedef __attribute__((address_space(1))) uint32_t g32;
    typedef __attribute__((address_space(1))) uint64_t g64;
    const uintptr_t base = reinterpret_cast<uintptr_t>(c16);
    auto put = [&](uint32_t sz) {  // bytes [lo, lo + sz), lo aligned to sz
        const uint64_t v = lo < 8 ? x0 >> (8 * lo) : x1 >> (8 * (lo - 8));
        const uintptr_t p = base + lo;
        if (sz == 8) *reinterpret_cast<g64*>(p) = v;
        else if (sz == 4) *reinterpret_cast<g32*>(p) = (uint32_t)v;
        else if (sz == 2) *reinterpret_cast<g16*>(p) = (uint16_t)v;
        else *reinterpret_cast<g8*>(p) = (uint8_t)v;
        lo += sz;
    };
    if ((lo & 1) && lo + 1 <= hi) put(1);
    if ((lo & 2) && lo + 2 <= hi) put(2);
    if ((lo & 4) && lo + 4 <= hi) put(4);
    if (lo + 8 <= hi) put(8);
    if (lo + 4 <= hi) put(4);
    if (lo + 2 <= hi) put(2);
    if (lo + 1 <= hi) put(1);
}

// s_waitcnt needs an immediate: wait until at most min(c, 8) / min(c, 63) vector-memory
// operations are outstanding (a smaller count than the true number of younger operations only
// waits longer). Two ladders: one function taking the cap compiled to different code in the
// fill pass and the words decoder.
__device__ __forceinline__ void vmcnt_at_most(uint32_t c) {
    switch (c) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    }
}
__device__ __forceinline__ void vmcnt_at_most63(uint32_t c) {
#define CPK_VM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
#define CPK_VM8(B) CPK_VM(B) CPK_VM(B + 1) CPK_VM(B + 2) CPK_VM(B + 3) CPK_VM(B + 4) CPK_VM(B + 5) CPK_VM(B + 6) CPK_VM(B + 7)
    switch (c < 63u ? c : 63u) {
        CPK_VM8(0) CPK_VM8(8) CPK_VM8(16) CPK_VM8(24) CPK_VM8(32) CPK_VM8(40) CPK_VM8(48)
        CPK_VM(56) CPK_VM(57) CPK_VM(58) CPK_VM(59) CPK_VM(60) CPK_VM(61) CPK_VM(62)
        default: asm volatile("s_waitcnt vmcnt(63)" ::: "memory"); break;
    }
#undef CPK_VM8
#undef CPK_VM
}

}  // namespace cpk
