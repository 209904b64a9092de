// tests/host_walk/stubs/kernels/device_helpers.h
// The two functions of capnp-zig_amd/csrc/kernels/device_helpers.h that the message walker uses;
// the rest of that header is wave intrinsics, which no host compiler takes.
// tests/test_walk_fuzz.py asserts that both functions are, character for character, the real
// header's: change them there and copy them here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpk {

__device__ __forceinline__ uint64_t gload64(const uint8_t* p) {
    return *reinterpret_cast<const uint64_t*>(p);
}

__device__ __forceinline__ int64_t ptr_offset_words(uint64_t w) {  // message.zig:11-18
    const uint32_t raw = (uint32_t)((w >> 2) & 0x3FFFFFFFu);
    return (raw & 0x20000000u) ? (int64_t)raw - ((int64_t)1 << 30) : (int64_t)raw;
}

}  // namespace cpk
