// Multi-row GEMV kernel and launchers (templates) shared by gemv_rows_{f16,f32,i8}.hip, which
// instantiate rows_launch_epi<WT> (split by weight type so the build compiles them in parallel).
#pragma once
#include "gemv_rows_impl.h"

namespace llmi {
namespace gemv_detail {

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, int kUnroll, bool XFIX, int M>
__global__ __launch_bounds__(kThreads) void gemv_rows_kernel(GemvRowsArgs p) {
    extern __shared__ __attribute__((aligned(16))) float4 xs[];
    gemv_rows_body<WT, ROWS, EPI, NORM, GT, kUnroll, XFIX, M>(p, blockIdx.x, gridDim.x, xs);
}

inline int rows_device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
    }
    return cus;
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, bool XF, int M>
int rows_launch_k(const GemvRowsArgs& p, int grid, hipStream_t s) {
    auto kern = gemv_rows_kernel<WT, ROWS, EPI, NORM, GT, kRowsUnroll, XF, M>;
    const GemvArgs& a = p.a;
    const int kl = (EPI == EPI_ATOMIC) ? a.k / a.ksplit : a.k;
    const size_t lds = gemv_rows_lds_bytes(kl, M);
    LLMI_REQUIRE(lds <= (size_t)LLMI_ROWS_MAX_LDS, "gemv_rows: the x images exceed the LDS");
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 LLMI_ROWS_MAX_LDS) == hipSuccess;
    LLMI_REQUIRE(attr, "gemv_rows: cannot raise the dynamic LDS limit");
    // clamp an automatic grid to what is resident (gemv_launch.h launch_k); argmax grids stay:
    // their partial count is gemv_grid's
    if (EPI != EPI_ARGMAX && a.grid == 0) {
        static size_t occ_lds = ~(size_t)0;
        static int occ_blocks = 0;
        if (lds != occ_lds) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kern), kThreads, lds) !=
                hipSuccess)
                n = 0;
            occ_blocks = n * rows_device_cus();
            occ_lds = lds;
        }
        const int S = (EPI == EPI_ATOMIC) ? a.ksplit : 1;
        if (occ_blocks >= S && grid > occ_blocks) grid = occ_blocks / S * S;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, s, p);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, bool XF>
int rows_launch_m(const GemvRowsArgs& p, int grid, hipStream_t s) {
    switch (p.m) {
        case 2: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 2>(p, grid, s);
        case 3: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 3>(p, grid, s);
        case 4: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 4>(p, grid, s);
        case 5: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 5>(p, grid, s);
        case 6: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 6>(p, grid, s);
        case 7: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 7>(p, grid, s);
        case 8: return rows_launch_k<WT, ROWS, EPI, NORM, GT, XF, 8>(p, grid, s);
    }
    LLMI_REQUIRE(false, "gemv_rows: m must be 2..8");
}

// the input forms of the token step: a plain fp32 x, or the fixed-point residual with its RMSNorm
template <typename WT, int ROWS, int EPI>
int rows_launch_in(const GemvRowsArgs& p, int grid, hipStream_t s) {
    const GemvArgs& a = p.a;
    const bool fixed = p.row[0].x_fixed != nullptr;
    if (!fixed && a.gamma == nullptr) return rows_launch_m<WT, ROWS, EPI, false, float, false>(p, grid, s);
    if constexpr (EPI == EPI_STORE || EPI == EPI_SILU_MUL || EPI == EPI_ARGMAX) {
        if (fixed && a.gamma != nullptr) {
            if (a.g_dtype == LLMI_F16) return rows_launch_m<WT, ROWS, EPI, true, __half, true>(p, grid, s);
            if (a.g_dtype == LLMI_F32) return rows_launch_m<WT, ROWS, EPI, true, float, true>(p, grid, s);
            LLMI_REQUIRE(false, "gemv_rows: gamma dtype must be f16 or f32");
        }
    }
    return rows_unsupported("x is either fp32 without rmsnorm, or fixed point with rmsnorm and a store / silu / "
                            "argmax epilogue");
}

template <typename WT>
int rows_launch_epi(const GemvRowsArgs& p, int grid, hipStream_t s) {
    switch (p.a.epi) {
        case EPI_STORE: return rows_launch_in<WT, kRows, EPI_STORE>(p, grid, s);
        case EPI_ADD: return rows_launch_in<WT, kRows, EPI_ADD>(p, grid, s);
        case EPI_SILU_MUL: return rows_launch_in<WT, 2, EPI_SILU_MUL>(p, grid, s);
        case EPI_ARGMAX: return rows_launch_in<WT, kRows, EPI_ARGMAX>(p, grid, s);
        case EPI_ATOMIC: return rows_launch_in<WT, kRows, EPI_ATOMIC>(p, grid, s);
    }
    LLMI_REQUIRE(false, "gemv_rows: bad epilogue");
}

}  // namespace gemv_detail
}  // namespace llmi
