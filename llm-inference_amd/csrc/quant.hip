// Weight quantisers. W4A16 (quantize_groups_i4_launch): further down, with its own notes.
// W8A16 quantiser: fp32 rows -> int8 q[r, :] and one fp16 scale per row, w ~= q * s
// (the format gemv_impl.h and gemm.hip dequantise; oracle/llama_ref.py: dequant).
//
// Per row r of w [rows, ld] (only the first row_len columns are data):
//   amax = max_j |w[r, j]|, j < row_len          (the whole row, also when only a slice is written)
//   s    = fp16_rne(amax / 127)                  (fp16 zero -> 2^-24, overflow -> 65504)
//   q[r, c] = clamp(rint(w[r, col0 + c] / s), -127, 127), c < cols      (q dense [rows, cols])
// Both divisions are the correctly rounded fp32 ones, rint is round-half-even, so a numpy
// restatement gives the same bits. A row with a NaN or an infinity gets s = 0, q = 0 and
// counts once in *bad_rows.
//
// One workgroup of 256 lanes per row. The row is read once with 16-byte loads and kept in
// registers (NV float4 per lane: rows up to NV * 1024 floats; the 13B model's longest row,
// 13,824 floats, takes 14) while the maximum goes through the wave butterfly and the four
// waves' LDS slots; the second pass quantises from those registers. Longer rows (NV = 0) are
// read a second time, from L2 where the first pass left them. A lane packs the four values
// of each float4 into one dword, so a wave's store instruction writes 256 contiguous bytes.
#include "kernels.h"

namespace llmi {
namespace {

constexpr int kQuantThreads = 256;

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }
__device__ __forceinline__ uint32_t abs_bits_max(const float4& v) {
    return max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w)));
}

// |w| as unsigned bits: ordered like the magnitudes, with every infinity and NaN at or above
// 0x7F800000 -- one integer maximum finds the row's amax and its non-finite values (fmaxf
// would drop a NaN)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t quant_pack4(const float4& v, float s) {
    auto q = [s](float x) -> uint32_t {
        const float r = fminf(fmaxf(rintf(__fdiv_rn(x, s)), -127.f), 127.f);
        return (uint32_t)(int)r & 0xFFu;
    };
    return q(v.x) | (q(v.y) << 8) | (q(v.z) << 16) | (q(v.w) << 24);
}

// n4 / c0 / c4: row_len, col0 and cols in float4 units
template <int NV>
__global__ __launch_bounds__(kQuantThreads) void quantize_rows_i8_kernel(const float* __restrict__ w, size_t ld,
                                                                        int n4, int c0, int c4,
                                                                        int8_t* __restrict__ q,
                                                                        __half* __restrict__ scales,
                                                                        int32_t* __restrict__ bad_rows) {
    __shared__ uint32_t red[kQuantThreads / kWave];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float4* wr = reinterpret_cast<const float4*>(w + row * ld);
    uint32_t* qr = reinterpret_cast<uint32_t*>(q + row * (size_t)c4 * 4);

    float4 v[NV > 0 ? NV : 1];
    uint32_t m = 0;
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = i * kQuantThreads + tid;
            v[i] = j < n4 ? wr[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            m = max(m, abs_bits_max(v[i]));
        }
    } else {
        for (int j = tid; j < n4; j += kQuantThreads) m = max(m, abs_bits_max(wr[j]));
    }
    m = wave_max_u32(m);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));

    const bool bad = m >= 0x7F800000u;
    unsigned short sb = 0;
    if (!bad) {
        sb = __half_as_ushort(__float2half_rn(__fdiv_rn(__uint_as_float(m), 127.0f)));
        if (sb == 0) sb = 1;                  // below half the smallest subnormal: 2^-24
        else if (sb == 0x7C00) sb = 0x7BFF;   // past the fp16 range: 65504
    }
    const __half sh = __ushort_as_half(sb);
    const float s = __half2float(sh);
    if (tid == 0) {
        scales[row] = sh;
        if (bad && bad_rows) atomicAdd(bad_rows, 1);
    }
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * kQuantThreads + tid - c0;
            if (c >= 0 && c < c4) qr[c] = bad ? 0u : quant_pack4(v[i], s);
        }
    } else {
        for (int c = tid; c < c4; c += kQuantThreads) qr[c] = bad ? 0u : quant_pack4(wr[c0 + c], s);
    }
}

// ---- W4A16: groups of 128 columns, one fp16 scale a group (format: include/llmi.h,
// llmi_quantize_groups_i4). Same plan as the int8 kernel: one workgroup a row, the row read once
// into registers (NV float4 a lane; NV = 0: longer rows, read again from L2). A group is 32
// float4 = half a wave: its maximum goes through the xor 16..1 butterfly, the row's non-finite
// check through the block maximum. A lane packs its float4 into four nibbles (2 bytes), so a
// wave's store writes 128 contiguous bytes.
__device__ __forceinline__ uint32_t half_wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned short group_scale_bits(uint32_t amax_bits) {
    unsigned short sb = __half_as_ushort(__float2half_rn(__fdiv_rn(__uint_as_float(amax_bits), 7.0f)));
    if (sb == 0) sb = 1;                  // below half the smallest subnormal: 2^-24
    else if (sb == 0x7C00) sb = 0x7BFF;   // past the fp16 range: 65504
    return sb;
}
__device__ __forceinline__ unsigned short quant_pack4_i4(const float4& v, float s) {
    auto q = [s](float x) -> uint32_t {
        const float r = fminf(fmaxf(rintf(__fdiv_rn(x, s)), -7.f), 7.f);
        return (uint32_t)((int)r + 8);
    };
    return (unsigned short)(q(v.x) | (q(v.y) << 4) | (q(v.z) << 8) | (q(v.w) << 12));
}

// n4: row_len in float4 units, a multiple of 32
template <int NV>
__global__ __launch_bounds__(kQuantThreads) void quantize_groups_i4_kernel(const float* __restrict__ w, size_t ld,
                                                                          int n4, uint8_t* __restrict__ q,
                                                                          __half* __restrict__ scales,
                                                                          int32_t* __restrict__ bad_rows) {
    __shared__ uint32_t red[kQuantThreads / kWave];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float4* wr = reinterpret_cast<const float4*>(w + row * ld);
    unsigned short* qr = reinterpret_cast<unsigned short*>(q + row * (size_t)n4 * 2);
    __half* sr = scales + row * (size_t)(n4 / 32);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 v[NV > 0 ? NV : 1];
    uint32_t m = 0;
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = i * kQuantThreads + tid;
            v[i] = j < n4 ? wr[j] : zero;
            m = max(m, abs_bits_max(v[i]));
        }
    } else {
        for (int j = tid; j < n4; j += kQuantThreads) m = max(m, abs_bits_max(wr[j]));
    }
    m = wave_max_u32(m);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
    __syncthreads();
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    const bool bad = m >= 0x7F800000u;
    if (tid == 0 && bad && bad_rows) atomicAdd(bad_rows, 1);

    // group j / 32 of the row: its scale from the half wave's maximum, then the lane's four nibbles
    // (j < n4 is uniform over a half wave: n4 is a multiple of 32)
    auto emit = [&](int j, const float4& x) {
        const unsigned short sb = bad ? (unsigned short)0 : group_scale_bits(half_wave_max_u32(abs_bits_max(x)));
        if (j < n4) {
            const __half sh = __ushort_as_half(sb);
            if ((tid & 31) == 0) sr[j >> 5] = sh;
            qr[j] = bad ? (unsigned short)0x8888 : quant_pack4_i4(x, __half2float(sh));
        }
    };
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) emit(i * kQuantThreads + tid, v[i]);
    } else {
        for (int j0 = 0; j0 < n4; j0 += kQuantThreads) {  // every lane takes every trip: the butterfly needs them
            const int j = j0 + tid;
            emit(j, j < n4 ? wr[j] : zero);
        }
    }
}

}  // namespace

int quantize_groups_i4_launch(const float* w, size_t ld, int rows, int row_len, uint8_t* q, __half* scales,
                              int32_t* bad_rows, hipStream_t s) {
    LLMI_REQUIRE(w && q && scales, "quantize_groups_i4: null pointer");
    LLMI_REQUIRE(rows >= 0 && row_len > 0 && row_len % 128 == 0,
                 "quantize_groups_i4: row_len must be a positive multiple of the 128-column group");
    LLMI_REQUIRE(ld % 4 == 0 && (size_t)row_len <= ld, "quantize_groups_i4: need row_len <= ld, ld a multiple of 4");
    LLMI_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)q % 4 == 0 && (uintptr_t)scales % 2 == 0 &&
                     (!bad_rows || (uintptr_t)bad_rows % 4 == 0),
                 "quantize_groups_i4: w must be 16-byte aligned, q and bad_rows 4-byte, scales 2-byte");
    if (rows == 0) return LLMI_OK;
    const int n4 = row_len / 4;
    const dim3 grid(rows), block(kQuantThreads);
    if (n4 <= 4 * kQuantThreads)
        quantize_groups_i4_kernel<4><<<grid, block, 0, s>>>(w, ld, n4, q, scales, bad_rows);
    else if (n4 <= 16 * kQuantThreads)
        quantize_groups_i4_kernel<16><<<grid, block, 0, s>>>(w, ld, n4, q, scales, bad_rows);
    else
        quantize_groups_i4_kernel<0><<<grid, block, 0, s>>>(w, ld, n4, q, scales, bad_rows);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int quantize_rows_i8_launch(const float* w, size_t ld, int rows, int row_len, int col0, int cols, int8_t* q,
                            __half* scales, int32_t* bad_rows, hipStream_t s) {
    LLMI_REQUIRE(w && q && scales, "quantize_rows_i8: null pointer");
    LLMI_REQUIRE(rows >= 0 && row_len > 0 && col0 >= 0 && cols > 0, "quantize_rows_i8: bad shape");
    LLMI_REQUIRE(ld % 4 == 0 && row_len % 4 == 0 && col0 % 4 == 0 && cols % 4 == 0,
                 "quantize_rows_i8: ld, row_len, col0 and cols must be multiples of 4");
    LLMI_REQUIRE((size_t)col0 + (size_t)cols <= (size_t)row_len && (size_t)row_len <= ld,
                 "quantize_rows_i8: need col0 + cols <= row_len <= ld");
    LLMI_REQUIRE((uintptr_t)w % 16 == 0 && (uintptr_t)q % 4 == 0 && (uintptr_t)scales % 2 == 0 &&
                     (!bad_rows || (uintptr_t)bad_rows % 4 == 0),
                 "quantize_rows_i8: w must be 16-byte aligned, q and bad_rows 4-byte, scales 2-byte");
    if (rows == 0) return LLMI_OK;
    const int n4 = row_len / 4, c0 = col0 / 4, c4 = cols / 4;
    const dim3 grid(rows), block(kQuantThreads);
    if (n4 <= 4 * kQuantThreads)
        quantize_rows_i8_kernel<4><<<grid, block, 0, s>>>(w, ld, n4, c0, c4, q, scales, bad_rows);
    else if (n4 <= 8 * kQuantThreads)
        quantize_rows_i8_kernel<8><<<grid, block, 0, s>>>(w, ld, n4, c0, c4, q, scales, bad_rows);
    else if (n4 <= 16 * kQuantThreads)
        quantize_rows_i8_kernel<16><<<grid, block, 0, s>>>(w, ld, n4, c0, c4, q, scales, bad_rows);
    else
        quantize_rows_i8_kernel<0><<<grid, block, 0, s>>>(w, ld, n4, c0, c4, q, scales, bad_rows);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace llmi
