// tests/host_walk/stubs/hip/hip_runtime.h
// What kernels/message_walk.h and kernels/list_read.h need of <hip/hip_runtime.h> to compile for
// the host with a plain C++ compiler: the qualifiers defined away (`__shared__` becomes a static
// array of the one host thread) and threadIdx / blockIdx as variables the driver sets per unit.
#pragma once
#include <stdint.h>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static

struct HostWalkDim3 {
    uint32_t x, y, z;
};
static HostWalkDim3 threadIdx, blockIdx;

static inline void __syncthreads() {}
