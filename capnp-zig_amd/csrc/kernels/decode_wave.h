// kernels/decode_wave.h
// The window machinery and the decode fallback built on it. A window of kWvWin packed bytes in a
// wave's LDS slice: staged (WvWin, wv_stage), its record chain found by speculative walks and
// verification rounds (wv_len, wv_walk, wv_resolve), counted (wv_count) and expanded (wv_expand).
// decode_wave_kernel<kWvMarked / kWvLong> walks a unit window after window, a wave per unit: the
// serial list's long units and the units the read-message passes mark. The long-unit decoder, the
// framer and the splitter run the same machinery a window per wave. DESIGN.md §2.3 (the fallback),
// §2.6 (long units).
// Leans on:
//   common.h             kWave, kStNeedFull, the ST_* statuses
//   device_helpers.h     lane_id, stage_linear, ld_u64, lds_u64_at, perm64, expand_selector,
//                        readlane, wave_incl_sum, wave_lds_sync
//   class_ws.h           the serial list: kSlotSerial, serial_off
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "class_ws.h"
#include "kernels/common.h"
#include "kernels/device_helpers.h"

namespace cpk {

// ---------------------------------------------------------------------------
// DECODE fallback, wave per unit (long units of the indexed decoder, marked units
// of the read-message passes; profiles/r01_decode_experiments.md)
// ---------------------------------------------------------------------------
// One wave owns one unit. The unit's packed bytes are processed in windows of
// up to kWvWin bytes (one window for units up to ~4.5 KiB packed), each staged
// in the wave's LDS slice with coalesced 16-B loads. Lane j owns the chunk
// [j*C, (j+1)*C) of the window and must find the true record chain through it
// (tag -> record length -> next tag, message.zig:152-191), which is serial:
//
//   walk A   every lane walks its chunk from the chunk start (a guess),
//            marking the tags it visits in a per-byte mark array (walk id 1);
//   walk B   every lane walks from the exit of its left neighbour's walk A
//            (the neighbour's guess of where the chain enters this chunk),
//            stopping as soon as it reaches a marked tag: from there the
//            chain is the marked walk's, so its exit is known (walk id 2);
//   rounds   lane j is verified when its entry equals lane j-1's exit and
//            lane j-1 is verified (lane 0 enters at 0, the window start is a
//            tag). Every lane whose entry disagrees re-walks from its
//            neighbour's exit, again stopping at the first marked tag. Each
//            round verifies at least the first disagreeing lane, so this ends
//            in <= 64 rounds; because chains from different entries couple
//            within a few records, 0-2 rounds are typical.
//   count    each lane sums the output words of its verified records; a wave
//            scan gives every lane its output word offset;
//   expand   each lane expands its records (v_perm_b32 scatter of the nonzero
//            bytes) and stores the words; zero runs and literal runs longer
//            than a few words are handed to the whole wave (coalesced).
//
// The window's exit (lane 63's verified exit) is the next window's start, so
// any unit size works; LDS-resident chunks keep every chain step an LDS read.
constexpr uint32_t kWvWaves = 4;                      // waves (units) per block
constexpr uint32_t kWvBlock = kWvWaves * kWave;
constexpr uint32_t kWvWin = 4608;                     // packed bytes per window (64 chunks x 72 B)
constexpr uint32_t kWvPk = kWvWin + 64;               // + 15 B alignment slack + 16 B overshoot + read slack
constexpr uint32_t kWvCmin = 32;                      // minimum chunk bytes per lane
constexpr uint32_t kWvStageK = (kWvPk / 16 + 63) / 64;
constexpr uint32_t kEOFX = 0xFFFFFFFFu;               // "the chain ran past the end of the input"
constexpr uint32_t kWvExtLane = 3;                    // longer literal runs are listed by the whole wave
constexpr uint32_t kWvList = 1024;                    // output words per expand pass (u16 list in the mark array)
constexpr uint32_t kPosMask = 0x1FFFu;                // list code: window position (< 8192)
constexpr uint32_t kLit = 0x2000u;                    // list code: literal word (identity selector)
constexpr uint32_t kZero = 0x8000u;                   // list code: zero word
constexpr uint32_t kZero2 = kZero | (kZero << 16);
static_assert(kWvList * 2 <= kWvWin, "list aliases the mark array");
static_assert(kWvWin + 16 + 2058 < 8192, "list codes hold window positions");
constexpr uint32_t kWvSlack = 16;                     // plausible entry offset into a chunk (records are <= 9 B)

__device__ __forceinline__ uint32_t wv_sel_exit(uint32_t m, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t e4,
                                                uint32_t e5, uint32_t e6, uint32_t e7) {
    uint32_t r = e7;
    r = (m == 6) ? e6 : r;
    r = (m == 5) ? e5 : r;
    r = (m == 4) ? e4 : r;
    r = (m == 3) ? e3 : r;
    r = (m == 2) ? e2 : r;
    r = (m == 1) ? e1 : r;
    return r;
}

// Walk the chain from window position r to the first tag position >= cend,
// marking visited tags with id (id 0: no marks). Stops at a tag marked by an
// earlier walk and reports its id in hit (the caller maps it to that walk's
// exit). Returns kEOFX if a record runs past the input end (rem bytes).
__device__ __forceinline__ uint32_t wv_len(uint32_t t, uint32_t c) {  // record length for tag t
    const uint32_t zf = (t == 0u) | (t == 0xFFu);             // 00 -> 2, FF -> 10 + 8c, else 1 + popc
    return 1u + __popc(t) + zf + ((t == 0xFFu) ? 8u * c : 0u);
}

__device__ __forceinline__ uint32_t wv_walk(const uint8_t* pk, uint8_t* mk, uint32_t sh, uint32_t rem, uint32_t r,
                                            uint32_t cend, uint32_t id, uint32_t& hit) {
    uint32_t h = 0;
    bool go = r < cend;
    while (go) {  // body is branch-free: one loop exit
        uint32_t m = mk[r];
        uint32_t t = pk[sh + r];
        uint32_t c = pk[sh + r + 9];
        asm volatile("" : "+v"(m), "+v"(t), "+v"(c));  // issue the three LDS reads together, one wait
        const uint32_t len = wv_len(t, c);
        const bool coupled = m != 0;
        mk[r] = (uint8_t)(coupled ? m : id);  // unconditional: rewrites m where coupled or id == 0
        h = m;
        const uint32_t nr = (r + len > rem) ? kEOFX : r + len;
        r = coupled ? r : nr;
        go = !coupled && r < cend;
    }
    hit = h;
    return r;
}

// A window of a unit's packed bytes staged in the wave's LDS slice: window byte r (unit
// byte X + r) at pk[sh + r] for r < nload. Records starting in [0, Pw) belong to the
// window; nload adds the <= 9 bytes such a record reaches past Pw.
struct WvWin {
    const uint8_t* g;  // unit byte X
    uint32_t sh;       // g & 15
    uint32_t rem;      // unit bytes from X on (clamped to 2^31 - 1)
    uint32_t Pw;       // window bytes
    uint32_t nload;    // staged bytes
};

// Stage window [X, X + kWvWin) of a unit of P packed bytes and clear its marks.
__device__ __forceinline__ WvWin wv_stage(uint8_t* pk, uint8_t* mk, const uint8_t* src, uint64_t P, uint64_t X,
                                          uint32_t lane) {
    WvWin w;
    const uint64_t rem64 = P - X;
    w.rem = rem64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)rem64;
    w.Pw = min(w.rem, kWvWin);
    w.nload = min(w.rem, w.Pw + 16);
    w.g = src + X;
    w.sh = (uint32_t)(reinterpret_cast<uintptr_t>(w.g) & 15);
    wave_lds_sync();
    stage_linear<kWvStageK>(pk, w.g - w.sh, (w.sh + w.nload + 15) >> 4, lane);
    for (uint32_t i = lane * 16; i < w.Pw; i += 16 * kWave) *reinterpret_cast<uint4*>(mk + i) = make_uint4(0, 0, 0, 0);
    wave_lds_sync();
    return w;
}

// The record chain through a staged window whose first record starts at window byte d0
// (lane 0's entry, exact). Lane j owns the chunk [cs, ce); on return `ent` is the verified
// record start where the chain enters it, and the result is the window's exit: the first
// record start at or past Pw (window-relative), or kEOFX when a record runs past the
// unit's end (walks A and B and the verification rounds: see above).
__device__ __forceinline__ uint32_t wv_resolve(const uint8_t* pk, uint8_t* mk, const WvWin& w, uint32_t d0,
                                               uint32_t lane, uint32_t& ent, uint32_t& cs, uint32_t& ce) {
    const uint32_t C = max(kWvCmin, (w.Pw + 63) >> 6);
    cs = min(lane * C, w.Pw);
    ce = min(cs + C, w.Pw);

    // ---- walk A: lane 0 from d0, every other lane from its chunk start (a guess) -----
    const uint32_t a0 = lane == 0 ? d0 : cs;
    uint32_t hit;
    const uint32_t e1 = wv_walk(pk, mk, w.sh, w.rem, a0, ce, 1, hit);
    uint32_t e2 = 0, e3 = 0, e4 = 0, e5 = 0, e6 = 0, e7 = 0;

    // ---- walk B: enter where the left neighbour's walk A left off ---------------------
    // An entry far past the chunk start (a misread FF run, or a misread record running
    // past the input end) would only pass through; keep walk A's guess.
    ent = __shfl_up(e1, 1, kWave);
    if (lane == 0) ent = d0;
    else if (ent > cs + kWvSlack) ent = cs;
    uint32_t ex = e1;
    if (ent != a0) {
        ex = wv_walk(pk, mk, w.sh, w.rem, ent, ce, 2, hit);
        if (hit) ex = wv_sel_exit(hit, e1, e2, e3, e4, e5, e6, e7);
        e2 = ex;
    }

    // ---- verification rounds ------------------------------------------------------------
    // Lanes before the first disagreeing lane f are verified. A disagreeing lane re-walks
    // from its neighbour's exit when that neighbour is verified (lane f), or when the
    // neighbour agrees with ITS neighbour this round and the exit is a plausible entry
    // (<= kWvSlack into the chunk): far or EOF exits adopted from an unverified neighbour
    // would otherwise ripple one lane per round.
    uint32_t nid = 3;
    for (;;) {
        uint32_t prev = __shfl_up(ex, 1, kWave);
        if (lane == 0) prev = d0;
        const bool bad = ent != prev;
        const uint64_t bm = __ballot(bad);
        if (!bm) break;
        const uint32_t f = (uint32_t)__builtin_ctzll(bm);
        const bool left_bad = lane > 0 && ((bm >> (lane - 1)) & 1);
        if (bad && (lane == f || (!left_bad && prev <= cs + kWvSlack))) {
            ent = prev;
            const uint32_t id = nid <= 7 ? nid : 0;
            ex = wv_walk(pk, mk, w.sh, w.rem, ent, ce, id, hit);
            if (hit) ex = wv_sel_exit(hit, e1, e2, e3, e4, e5, e6, e7);
            e3 = (id == 3) ? ex : e3;
            e4 = (id == 4) ? ex : e4;
            e5 = (id == 5) ? ex : e5;
            e6 = (id == 6) ? ex : e6;
            e7 = (id == 7) ? ex : e7;
            ++nid;
        }
    }
    return readlane(ex, kWave - 1);
}

// Output words of a lane's verified records [ent, ce).
__device__ __forceinline__ uint32_t wv_count(const uint8_t* pk, uint32_t sh, uint32_t ent, uint32_t ce) {
    uint32_t words = 0;
    for (uint32_t r = ent; r < ce;) {
        uint32_t t = pk[sh + r];
        uint32_t b1 = pk[sh + r + 1];
        uint32_t c9 = pk[sh + r + 9];
        asm volatile("" : "+v"(t), "+v"(b1), "+v"(c9));
        words += 1u + ((t == 0u) ? b1 : 0u) + ((t == 0xFFu) ? c9 : 0u);
        r += wv_len(t, c9);
    }
    return words;
}

// Expand the window's verified records into o[0 .. total): lane records produce words
// [wbeg, wend). Passes of kWvList output words:
//   list:   each lane walks its verified records once more and writes, for every output
//           word of the pass that its records produce, a 16-bit source code into a list
//           in LDS (the mark array, dead by now): code = q (window position of a tag;
//           word = perm(bytes q+1..q+8, lut[byte q])) or kLit | (s - 1) (literal word at
//           bytes s..s+7); zero-run words keep the kZero code the list is reset to;
//   expand: lane i turns list entry i into its word and stores it, so every store
//           instruction writes 64 consecutive output words (512 B).
__device__ __forceinline__ void wv_expand(const uint8_t* pk, uint8_t* mk, const uint64_t* lut, const WvWin& w,
                                          uint32_t ent, uint32_t ce, uint32_t wbeg, uint32_t wend, uint32_t total,
                                          uint64_t* o, uint32_t lane) {
    const uint32_t sh = w.sh;
    uint16_t* const list = reinterpret_cast<uint16_t*>(mk);
    for (uint32_t W0 = 0; W0 < total; W0 += kWvList) {
        const uint32_t W1 = min(total, W0 + kWvList);
        wave_lds_sync();
        for (uint32_t i = lane * 8; i < kWvList; i += 8 * kWave)
            *reinterpret_cast<uint4*>(list + i) = make_uint4(kZero2, kZero2, kZero2, kZero2);
        wave_lds_sync();
        uint32_t pn = 0, ps = 0, pw = 0;  // long literal run handed to the wave
        if (wbeg < W1 && wend > W0) {
            uint32_t wo = wbeg;
            for (uint32_t r = ent; r < ce && wo < W1;) {
                uint32_t t = pk[sh + r];
                uint32_t b1 = pk[sh + r + 1];
                uint32_t c9 = pk[sh + r + 9];
                asm volatile("" : "+v"(t), "+v"(b1), "+v"(c9));
                const bool z = t == 0, f = t == 0xFFu;
                if (!z && wo >= W0) list[wo - W0] = (uint16_t)r;
                if (f && c9) {  // literal words r+10 .. r+10+8c
                    if (c9 <= kWvExtLane || pn != 0) {  // one long run per lane goes to the wave
                        for (uint32_t i = 0; i < c9; ++i) {
                            const uint32_t wi = wo + 1 + i;
                            if (wi >= W0 && wi < W1) list[wi - W0] = (uint16_t)(kLit | (r + 9 + 8 * i));
                        }
                    } else {
                        pn = c9;
                        ps = r + 9;
                        pw = wo + 1;
                    }
                }
                wo += 1u + (z ? b1 : 0u) + (f ? c9 : 0u);
                r += wv_len(t, c9);
            }
        }
        uint64_t pm = __ballot(pn != 0);
        while (pm) {  // long literal runs: the whole wave fills their entries
            const uint32_t l = (uint32_t)__builtin_ctzll(pm);
            pm &= pm - 1;
            const uint32_t nn = readlane(pn, l), ss = readlane(ps, l), ww = readlane(pw, l);
            for (uint32_t i = lane; i < nn; i += kWave) {
                const uint32_t wi = ww + i;
                if (wi >= W0 && wi < W1) list[wi - W0] = (uint16_t)(kLit | (ss + 8 * i));
            }
        }
        wave_lds_sync();
        for (uint32_t i = W0 + lane; i < W1; i += kWave) {
            const uint32_t code = list[i - W0];
            const uint32_t q = code & kPosMask;
            const bool lit = (code & kLit) != 0;
            uint64_t word = 0;
            if (!(code & kZero)) {
                if (!lit || q + 9 <= w.nload) {  // a tag's bytes are always staged
                    const uint32_t t = lit ? 0xFFu : pk[sh + q];
                    word = perm64(lds_u64_at(pk, sh + q + 1), lut[t]);
                } else {  // literal word past the staged bytes (long FF run), inside the input
                    word = ld_u64(w.g + q + 1);
                }
            }
            __builtin_nontemporal_store(word, o + i);  // streaming output (as the fill pass)
        }
    }
}

// SEL: kWvMarked the units a first pass marked kStNeedFull (the read-message passes, the words
// decoder's units stopped at their capacity; q, when given, counts them: 0 returns at once);
// kWvLong the long units the window table could not hold (the serial list that
// long_windows_kernel fills), one after another.
constexpr int kWvMarked = 1, kWvLong = 2;

template <int SEL>
__global__ __launch_bounds__(kWvBlock) void decode_wave_kernel(const uint8_t* __restrict__ in,
                                                               const uint64_t* __restrict__ in_off,
                                                               const uint64_t* __restrict__ in_len, uint32_t n,
                                                               uint8_t* __restrict__ out,
                                                               const uint64_t* __restrict__ out_off,
                                                               const uint64_t* __restrict__ out_cap,
                                                               uint64_t* __restrict__ out_len,
                                                               int32_t* __restrict__ status, uint32_t* q) {
    __shared__ __attribute__((aligned(16))) uint8_t pk_all[kWvWaves * kWvPk];
    __shared__ __attribute__((aligned(16))) uint8_t mk_all[kWvWaves * kWvWin];
    __shared__ uint64_t lut[256];  // tag -> v_perm selector that scatters the packed bytes (FF: identity, 00: zero)
    constexpr bool CK = SEL == kWvMarked;
    if (CK && q && *q == 0) return;  // kWvMarked with a count of marked units: none
    const bool QD = SEL == kWvLong;
    if (QD && q[kSlotSerial] == 0) return;  // no serial units (block-uniform)
    lut[threadIdx.x] = expand_selector(threadIdx.x);
    __syncthreads();
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t* pk = pk_all + wave * kWvPk;
    uint8_t* mk = mk_all + wave * kWvWin;
    // CK: a first pass ran; this kernel takes only the units it marked kStNeedFull, with a
    // small grid striding over the batch (64 statuses per load). QD: the serial list, a
    // wave per entry striding over it (no shared atomic cursor: contended takes serialise).
    const uint32_t* const serial = q + serial_off(n);
    const uint32_t nq = QD ? q[kSlotSerial] : n;
    const uint32_t stride = QD ? gridDim.x * kWvWaves : gridDim.x * kWvWaves * kWave;
    for (uint32_t ubase = QD ? blockIdx.x * kWvWaves + wave : (blockIdx.x * kWvWaves + wave) * kWave; ubase < nq;
         ubase += stride) {
    uint64_t todo = 1;
    if (CK) {
        const uint32_t u = ubase + lane;
        todo = __ballot(u < n && status[u] == kStNeedFull);
    }
    while (todo) {  // wave-uniform
    const uint32_t unit = CK ? ubase + (uint32_t)__builtin_ctzll(todo) : __builtin_amdgcn_readfirstlane(serial[ubase]);
    todo &= todo - 1;
    const uint8_t* src = in + in_off[unit];
    const uint64_t P = in_len[unit];
    uint8_t* dstb = out + out_off[unit];
    const uint64_t capw = out_cap[unit] >> 3;
    if (reinterpret_cast<uintptr_t>(dstb) & 7) {
        if (lane == 0) {
            out_len[unit] = 0;
            status[unit] = ST_ARG;
        }
        continue;
    }
    uint64_t* const dst = reinterpret_cast<uint64_t*>(dstb);

    uint64_t X = 0;   // packed position of the current window (always a tag)
    uint64_t Wb = 0;  // output words before the current window
    int32_t st = ST_OK;
    bool fits = true;
    if (QD) {
        // a counting walk first (the serial units are the rare ones the window table
        // cannot hold): a truncated or oversized unit writes nothing, as unpackPacked
        // returns its error before any output (message.zig:88-145)
        while (X < P) {
            const WvWin w = wv_stage(pk, mk, src, P, X, lane);
            uint32_t ent, cs, ce;
            const uint32_t xw = wv_resolve(pk, mk, w, 0, lane, ent, cs, ce);
            if (xw == kEOFX) {
                st = ST_EOF;
                break;
            }
            const uint32_t words = wv_count(pk, w.sh, ent, ce);
            Wb += readlane(wave_incl_sum(words), kWave - 1);
            X += xw;
        }
        if (st != ST_OK || Wb > capw) {
            if (lane == 0) {
                out_len[unit] = st == ST_OK ? 8 * Wb : 0;
                status[unit] = st != ST_OK ? st : ST_SPACE;
            }
            continue;
        }
        X = 0;
        Wb = 0;
    }
    while (X < P) {
        const WvWin w = wv_stage(pk, mk, src, P, X, lane);
        uint32_t ent, cs, ce;
        const uint32_t xw = wv_resolve(pk, mk, w, 0, lane, ent, cs, ce);
        if (xw == kEOFX) {
            st = ST_EOF;
            break;
        }
        const uint32_t words = wv_count(pk, w.sh, ent, ce);
        const uint32_t incl = wave_incl_sum(words);
        const uint32_t total = readlane(incl, kWave - 1);
        if (Wb + total > capw) fits = false;
        if (fits) wv_expand(pk, mk, lut, w, ent, ce, incl - words, incl, total, dst + Wb, lane);
        Wb += total;
        X += xw;
    }
    if (lane == 0) {
        out_len[unit] = (st == ST_OK) ? 8 * Wb : 0;
        status[unit] = (st != ST_OK) ? st : (fits ? ST_OK : ST_SPACE);
    }
    }  // marked units
    }  // unit loop
}

}  // namespace cpk
