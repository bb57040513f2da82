// GEMV launchers (templates) shared by the per-weight-dtype translation units
// gemv_f16.hip / gemv_f32.hip / gemv_i8.hip, which instantiate launch_epi<WT> (gemv_i4.hip specialises it)
// (split so the build compiles the dtypes in parallel).
#pragma once
#include "gemv_impl.h"
#include "xchg_impl.h"

namespace llmi {
namespace gemv_detail {


#ifndef LLMI_GEMV_MAX_GRID
#define LLMI_GEMV_MAX_GRID 1024
#endif
#ifndef LLMI_GEMV_MIN_WAVES
#define LLMI_GEMV_MIN_WAVES 1  // min waves per SIMD (launch-bounds 2nd arg): caps VGPRs
#endif

#ifndef LLMI_GEMV_MIN_WAVES_I8
// int8 at unroll <= 5: 4 waves per SIMD. The 13B-width q/k/v / gate_up / lm_head kernels need 130-135
// VGPRs (3 waves) for a prologue peak (the 5 x 16-B x-staging loads with gammas beside the first
// weight batch); capped at 128 they spill 2-4 VGPRs there and run 0.5 % faster a 13B token (same
// box, alternating libraries: 3,133 -> 3,115 us, profiles/r07i_int8_minwaves_ab.jsonl)
#define LLMI_GEMV_MIN_WAVES_I8 4
#endif
#ifndef LLMI_GEMV_MIN_WAVES_I4
// int4: a chunk is dotted against 8 float4 packets of x (32 VGPRs, shared by the wave's two rows),
// and hipcc hoists the packets of a whole batch: the kernels use 105-140 VGPRs (hipcc remarks;
// DESIGN.md §3, W4A16), so they get the 256-VGPR budget of 2 waves per SIMD instead of spilling
// under int8's cap of 128
#define LLMI_GEMV_MIN_WAVES_I4 2
#endif
template <typename WT, int U> constexpr int min_waves() {
    if (kIsI4<WT>) return LLMI_GEMV_MIN_WAVES_I4;
    return sizeof(WT) == 1 && U <= 5 ? LLMI_GEMV_MIN_WAVES_I8 : LLMI_GEMV_MIN_WAVES;
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, int XPT, int kUnroll, bool XFIX, int KPT = 1>
__global__ __launch_bounds__(kThreads, (min_waves<WT, kUnroll>())) void gemv_kernel(GemvArgs a) {
    // all LDS in one 16-B aligned dynamic region (cdna_hip_programming.md G17):
    // [PK][nc] float4 x image, then 16 floats of reduction scratch, then keys
    extern __shared__ __attribute__((aligned(16))) float4 xs[];
    WgStamp ts(a.stamps);
    gemv_body<WT, ROWS, EPI, NORM, GT, XPT, kUnroll, XFIX, PlainIO, KPT>(a, blockIdx.x, gridDim.x, xs);
    if constexpr (EPI == EPI_ATOMIC || EPI == EPI_ARGMAX) {  // TP: push yacc / the argmax keys from this launch
        const int k4 = (EPI == EPI_ATOMIC ? a.k / a.ksplit : a.k) / 4;
        xchg_detail::xchg_tail(a.xt, a.xt_cnt, reinterpret_cast<int*>(xs + k4) + 15);  // red[15]: free by now
    }
}

// Workgroups of one instantiation that fit the chip at once (occupancy x CUs),
// cached per instantiation and LDS size.
inline int device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
    }
    return cus;
}
template <typename WT, int ROWS, int EPI, bool NORM, typename GT, int XPT, int U, bool XF, int KPT = 1>
int launch_k(const GemvArgs& a, int grid, size_t lds, hipStream_t s) {
    auto kern = gemv_kernel<WT, ROWS, EPI, NORM, GT, XPT, U, XF, KPT>;
    // An automatic grid larger than what is resident leaves the excess workgroups to
    // start only when early ones retire -- a second, latency-bound round at the tail
    // (profiles/r01c: int8 13B q/k/v and down). Clamp it to the resident count
    // (argmax grids stay: their partial count is fixed by gemv_grid for step_start).
    if (EPI != EPI_ARGMAX && a.grid == 0 && a.kpar <= 1) {  // (kpar: one group per wave, no loop: never clamped)
        static size_t occ_lds = ~(size_t)0;
        static int occ_blocks = 0;
        if (lds != occ_lds) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kern), kThreads, lds) !=
                hipSuccess)
                n = 0;
            occ_blocks = n * device_cus();
            occ_lds = lds;
        }
        const int S = (EPI == EPI_ATOMIC) ? a.ksplit : 1;
        if (occ_blocks >= S && grid > occ_blocks) grid = occ_blocks / S * S;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, int U, bool XF>
int launch_u(const GemvArgs& a, int grid, hipStream_t s) {
    const int kl = (EPI == EPI_ATOMIC) ? a.k / a.ksplit : a.k;  // x extent one workgroup stages
    const size_t lds = gemv_lds_bytes(kl);
    const int k4 = kl / 4;
    const int xpt = gemv_xpt(k4);  // the staging width (gemv_impl.h)
    if constexpr ((EPI == EPI_STORE || EPI == EPI_SILU_MUL) && NORM && XF && U == 4) {
        // kpar (a TP rank's q/k/v and gate_up): the engine's normed fixed-point projections,
        // hidden <= 5120
        if (a.kpar > 1) {
            LLMI_REQUIRE(k4 <= 5 * kThreads, "gemv: kpar needs k <= 5120");
            if (a.kpar == 2)
                return xpt == 4 ? launch_k<WT, ROWS, EPI, NORM, GT, 4, U, XF, 2>(a, grid, lds, s)
                                : launch_k<WT, ROWS, EPI, NORM, GT, 5, U, XF, 2>(a, grid, lds, s);
            return xpt == 4 ? launch_k<WT, ROWS, EPI, NORM, GT, 4, U, XF, 4>(a, grid, lds, s)
                            : launch_k<WT, ROWS, EPI, NORM, GT, 5, U, XF, 4>(a, grid, lds, s);
        }
    }
    LLMI_REQUIRE(a.kpar <= 1, "gemv: kpar only for the engine's normed fixed-point q/k/v and gate_up");
    switch (xpt) {
        case 4: return launch_k<WT, ROWS, EPI, NORM, GT, 4, U, XF>(a, grid, lds, s);
        case 5: return launch_k<WT, ROWS, EPI, NORM, GT, 5, U, XF>(a, grid, lds, s);
        case 11: return launch_k<WT, ROWS, EPI, NORM, GT, 11, U, XF>(a, grid, lds, s);
        case 14: return launch_k<WT, ROWS, EPI, NORM, GT, 14, U, XF>(a, grid, lds, s);
    }
    return launch_k<WT, ROWS, EPI, NORM, GT, 0, U, XF>(a, grid, lds, s);
}

// the unroll gemv_pick_unroll (gemv_impl.h) chooses for this weight type and epilogue
template <typename WT, int EPI>
int pick_unroll(const GemvArgs& a, int groups) {
    return gemv_pick_unroll(WT_<WT>::EPL, EPI, a, groups);
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, bool XF>
int launch_x(const GemvArgs& a, int grid, int u, hipStream_t s) {
    if (u == 4) return launch_u<WT, ROWS, EPI, NORM, GT, 4, XF>(a, grid, s);
    if (u == 5) return launch_u<WT, ROWS, EPI, NORM, GT, 5, XF>(a, grid, s);
    return launch_u<WT, ROWS, EPI, NORM, GT, kUnrollMax, XF>(a, grid, s);
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT>
int launch_t(const GemvArgs& a, int grid, hipStream_t s) {
    static_assert(ROWS == (EPI == EPI_SILU_MUL ? 2 : kRows), "gemv_groups counts groups of these rows");
    const int u = pick_unroll<WT, EPI>(a, gemv_groups(a));
    if (a.x_fixed) {
        // the engine's residual stream is int64 fixed point: the normed projections read it
        if constexpr (NORM && EPI != EPI_ADD && EPI != EPI_ATOMIC) {
            return launch_x<WT, ROWS, EPI, NORM, GT, true>(a, grid, u, s);
        }
        LLMI_REQUIRE(false, "gemv: a fixed-point x needs rmsnorm and a store/silu/argmax epilogue");
    }
    return launch_x<WT, ROWS, EPI, NORM, GT, false>(a, grid, u, s);
}

template <typename WT, int ROWS, int EPI>
int launch_norm(const GemvArgs& a, int grid, hipStream_t s) {
    if (a.gamma == nullptr) return launch_t<WT, ROWS, EPI, false, float>(a, grid, s);
    if (a.g_dtype == LLMI_F16) return launch_t<WT, ROWS, EPI, true, __half>(a, grid, s);
    if (a.g_dtype == LLMI_F32) return launch_t<WT, ROWS, EPI, true, float>(a, grid, s);
    LLMI_REQUIRE(false, "gemv: gamma dtype must be f16 or f32");
}

template <typename WT>
int launch_epi(const GemvArgs& a, int grid, hipStream_t s) {
    switch (a.epi) {
        case EPI_STORE: return launch_norm<WT, kRows, EPI_STORE>(a, grid, s);
        case EPI_ADD: return launch_norm<WT, kRows, EPI_ADD>(a, grid, s);
        case EPI_SILU_MUL: return launch_norm<WT, 2, EPI_SILU_MUL>(a, grid, s);
        case EPI_ARGMAX: return launch_norm<WT, kRows, EPI_ARGMAX>(a, grid, s);
        case EPI_ATOMIC:
            LLMI_REQUIRE(a.gamma == nullptr, "gemv: the split-K atomic epilogue takes no rmsnorm");
            return launch_t<WT, kRows, EPI_ATOMIC, false, float>(a, grid, s);
    }
    LLMI_REQUIRE(false, "gemv: bad epilogue");
}


}  // namespace gemv_detail
}  // namespace llmi
