// What the whole-row kernels over a logits row share (nucleus.hip, logprob.hip): the 32-bit
// ordered key of a logit (the value half of argmax_key), the integer softmax weight
// w = rint((double)expf(z - m) * 2^32) -- sums of integers are exact in any order, which is
// what makes graph == eager and batch slot == single engine hold bitwise -- and the u64
// reductions of a 1024-lane workgroup.
#pragma once

#include "common.h"

namespace llmi {
namespace {

constexpr int kRowThreads = 1024;
constexpr int kRowWaves = kRowThreads / kWave;
constexpr unsigned long long kOne = 1ull << 32;

__device__ __forceinline__ uint32_t key_of(float z) { return (uint32_t)(argmax_key(z, 0u) >> 32); }
__device__ __forceinline__ float z_of(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ __forceinline__ unsigned long long weight_of(uint32_t key, uint32_t mkey, float m) {
    if (key == mkey) return kOne;  // also +inf and all -inf rows, where z - m is NaN
    return (unsigned long long)rint((double)expf(z_of(key) - m) * 4294967296.0);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long t = __shfl_up(v, off, kWave);
        if (lane >= off) v += t;
    }
    return v;
}
// red: kRowWaves u64 of LDS
__device__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int i = 0; i < kRowWaves; ++i) t += red[i];
    return t;
}

}  // namespace
}  // namespace llmi
