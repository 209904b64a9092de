// kernels/generate_scan.h
// The synthetic generator (generate_kernel) and the offsets scan
// (scan_local_kernel / scan_partials_kernel / scan_apply_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpk {

// ---------------------------------------------------------------------------
// synthetic generator and offset scan
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t unit, uint64_t word) {
    uint64_t x = seed ^ (unit * 0x9E3779B97F4A7C15ULL) ^ (word * 0xC2B2AE3D27D4EB4FULL);
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__global__ void generate_kernel(uint8_t* __restrict__ out, uint64_t n_units, uint64_t words_per_unit,
                                uint64_t unit_base, uint64_t seed, uint32_t thr) {
    const uint64_t total = n_units * words_per_unit;
    for (uint64_t gw = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; gw < total;
         gw += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t u = gw / words_per_unit, w = gw - u * words_per_unit;
        uint64_t h = mix64(seed, unit_base + u, w);
        uint64_t h2 = mix64(seed ^ 0xA5A5A5A5A5A5A5A5ULL, unit_base + u, w);
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t r = (uint32_t)(h >> (8 * k)) & 0xFF;
            uint32_t x = (uint32_t)(h2 >> (8 * k)) & 0xFF;
            uint64_t b = (r < thr) ? 0 : (1 + x % 255);
            v |= b << (8 * k);
        }
        *reinterpret_cast<uint64_t*>(out + 8 * gw) = v;
    }
}

constexpr int kScanItems = 8;
constexpr int kScanTile = 256 * kScanItems;

// block-local exclusive scan of u64 lengths; writes the block total to partial[blockIdx.x]
__global__ __launch_bounds__(256) void scan_local_kernel(const uint64_t* __restrict__ len, uint32_t n,
                                                         uint64_t* __restrict__ off,
                                                         uint64_t* __restrict__ partial) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + tid * kScanItems;
    uint64_t v[kScanItems];
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (base + k < n) ? len[base + k] : 0;
        t += v[k];
    }
    uint64_t x = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint64_t pre = 0;
    for (uint32_t q = 0; q < wave; ++q) pre += wsum[q];
    uint64_t run = pre + x - t;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) off[base + k] = run;
        run += v[k];
    }
    if (tid == 255) partial[blockIdx.x] = pre + x;
}

// single-block exclusive scan of the partials (in place), then base added
__global__ __launch_bounds__(1024) void scan_partials_kernel(uint64_t* __restrict__ partial, uint32_t np,
                                                             uint64_t base, uint64_t* __restrict__ off_last,
                                                             uint32_t n) {
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = base;
    __syncthreads();
    for (uint32_t b = 0; b < np; b += 1024) {
        uint64_t v = (b + tid < np) ? partial[b + tid] : 0;
        uint64_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint64_t pre = carry_s;
        for (uint32_t q = 0; q < wave; ++q) pre += wsum[q];
        if (b + tid < np) partial[b + tid] = pre + x - v;
        __syncthreads();
        if (tid == 1023) carry_s = pre + x;
        __syncthreads();
    }
    if (tid == 0) off_last[n] = carry_s;
}

__global__ __launch_bounds__(256) void scan_apply_kernel(uint64_t* __restrict__ off, uint32_t n,
                                                         const uint64_t* __restrict__ partial) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    const uint64_t add = partial[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) off[base + k] += add;
}

}  // namespace cpk
