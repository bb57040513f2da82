// GEMV instantiations for 4-bit group-quantised weights (LLMI_I4; see gemv.hip, gemv_launch.h and
// the format at llmi_quantize_groups_i4 in include/llmi.h).
//
// Only the three forms of a single-rank token step are instantiated (gemv.hip's gemv_check
// refuses the rest with LLMI_EUNSUPPORTED before anything is launched):
//   q/k/v     fixed-point x + RMSNorm (fp16 gamma), EPI_STORE
//   gate_up   the same input, EPI_SILU_MUL
//   down      fp32 x, EPI_ATOMIC with ksplit 1 (single producer or atomic add)
// A row is k / 2 bytes -- 128 16-B chunks at hidden 4096 -- so the unrolls are 2, 3 and 4
// (gemv_pick_unroll) instead of the 4, 5 and 8 of the wider dtypes.
#include "gemv_launch.h"

namespace llmi {
namespace gemv_detail {
namespace {

template <int ROWS, int EPI, bool NORM, int U, bool XF>
int launch_i4_xpt(const GemvArgs& a, int grid, hipStream_t s) {
    const size_t lds = gemv_lds_bytes(a.k);
    switch (gemv_xpt(a.k / 4)) {
        case 4: return launch_k<i4w, ROWS, EPI, NORM, __half, 4, U, XF>(a, grid, lds, s);
        case 5: return launch_k<i4w, ROWS, EPI, NORM, __half, 5, U, XF>(a, grid, lds, s);
        case 11: return launch_k<i4w, ROWS, EPI, NORM, __half, 11, U, XF>(a, grid, lds, s);
        case 14: return launch_k<i4w, ROWS, EPI, NORM, __half, 14, U, XF>(a, grid, lds, s);
    }
    return launch_k<i4w, ROWS, EPI, NORM, __half, 0, U, XF>(a, grid, lds, s);
}

template <int ROWS, int EPI, bool NORM, bool XF>
int launch_i4_u(const GemvArgs& a, int grid, hipStream_t s) {
    switch (gemv_pick_unroll(WT_<i4w>::EPL, EPI, a, gemv_groups(a))) {
        case 2: return launch_i4_xpt<ROWS, EPI, NORM, 2, XF>(a, grid, s);
        case 3: return launch_i4_xpt<ROWS, EPI, NORM, 3, XF>(a, grid, s);
    }
    return launch_i4_xpt<ROWS, EPI, NORM, 4, XF>(a, grid, s);
}

}  // namespace

template <>
int launch_epi<i4w>(const GemvArgs& a, int grid, hipStream_t s) {
    switch (a.epi) {
        case EPI_STORE: return launch_i4_u<kRows, EPI_STORE, true, true>(a, grid, s);
        case EPI_SILU_MUL: return launch_i4_u<2, EPI_SILU_MUL, true, true>(a, grid, s);
        case EPI_ATOMIC: return launch_i4_u<kRows, EPI_ATOMIC, false, false>(a, grid, s);
    }
    set_last_error("[llmi][ERROR] gemv: int4 weights have no kernel for this epilogue");
    return LLMI_EUNSUPPORTED;
}

}  // namespace gemv_detail
}  // namespace llmi
