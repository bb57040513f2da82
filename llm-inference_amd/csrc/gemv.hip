// HBM-streaming GEMV for batch-1 decode: y = W x, W [n_rows, k] row-major
// (fp16 / fp32 / int8+row-scale / int4+group-scale), x fp32, fp32 accumulate.
//
// Replaces launchLinearGemm -> cublasGemmEx with m = 1 (src/kernels/linear.cu:38-104,
// src/kernels/cublas_utils.cc:32-71) for the q/k/v, o, gate_up, down and lm_head
// projections.
//
// Roofline: HBM. Algorithmic bytes per launch = n_rows * k * sizeof(W) (+ scales);
// x (<= 55 KB) is L2-resident and re-read by every workgroup.
//
// Design (MI355X, wave64):
//  * one workgroup = 4 waves; x is staged once per workgroup into LDS in a
//    packet-major layout (packet p of chunk c at [p][c]) so that 64 lanes reading
//    consecutive chunks hit consecutive 16-byte slots (conflict-free ds_read_b128);
//  * a wave owns ROWS weight rows at a time and streams them with 16-byte
//    nontemporal loads, 8 loads per row in flight per lane (1 KiB per wave
//    instruction, coalesced), then a 6-step xor-shuffle reduction;
//  * prologue fusion: RMSNorm of x (modeling_llama.py:112-117) computed by every
//    workgroup from the L2-resident x -- removes the separate launchRMSNorm /
//    launchFusedAddBiasResidualRMSNorm kernels of self_decoder.cpp:59-70;
//  * epilogue fusion: residual add (add_residual.cu), SiLU*mul with the gate/up
//    row pair owned by one wave (act_kernel.cu:17-31), or logits + per-workgroup
//    argmax key for greedy sampling (topK.cu + sampling.cu with K = 1).
#include "gemv_impl.h"

namespace llmi {
namespace gemv_detail {
#ifndef LLMI_GEMV_MAX_GRID
#define LLMI_GEMV_MAX_GRID 1024
#endif
template <typename WT>
int launch_epi(const GemvArgs& a, int grid, hipStream_t s);  // gemv_{f16,f32,i8,i4}.hip
template <>
int launch_epi<i4w>(const GemvArgs& a, int grid, hipStream_t s);
}  // namespace gemv_detail

namespace {
using namespace gemv_detail;
int epl_of(int dt) { return dt == LLMI_F16 ? 8 : dt == LLMI_F32 ? 4 : dt == LLMI_I8 ? 16 : dt == LLMI_I4 ? 32 : 0; }

}  // namespace

int gemv_grid(const GemvArgs& a) {
    if (a.grid > 0) return a.grid;
    const int groups = gemv_groups(a);
    if (a.kpar > 1) return (groups + kWavesPerBlock / a.kpar - 1) / (kWavesPerBlock / a.kpar);  // a group per wave
    int blocks = (groups + kWavesPerBlock - 1) / kWavesPerBlock;
    // cap (default ~4 workgroups per CU on 256 CUs); waves then loop over several row groups
    const int S = (a.epi == EPI_ATOMIC) ? a.ksplit : 1;  // split-K: S workgroups per row-group block
    const int cap = LLMI_GEMV_MAX_GRID / S > 0 ? LLMI_GEMV_MAX_GRID / S : 1;
    return (blocks < cap ? blocks : cap) * S;
}

namespace {
// the argument contract of gemv_launch (and of gemv_plan, which launches nothing)
int gemv_check(const GemvArgs& a) {
    const int epl = epl_of(a.w_dtype);
    LLMI_REQUIRE(epl > 0, "gemv: weight dtype must be f16, f32, i8 or i4");
    if (a.w_dtype == LLMI_I4) {
        // int4 runs the three forms of a single-rank token step (gemv_i4.hip) and nothing else
        const bool proj = (a.epi == EPI_STORE || a.epi == EPI_SILU_MUL) && a.x_fixed && a.gamma && a.g_dtype == LLMI_F16;
        const bool down = a.epi == EPI_ATOMIC && a.x && !a.x_fixed && !a.gamma && a.ksplit == 1;
        if (!(proj || down) || a.kpar > 1 || a.y_tag || a.xt.buf || (a.ldw != 0 && a.ldw != a.k)) {
            set_last_error("[llmi][ERROR] gemv: int4 weights run a fixed-point x with an fp16 RMSNorm and the store or "
                           "silu epilogue, or an fp32 x with the atomic epilogue at ksplit 1; no kpar, granule rows, "
                           "exchange tail or ldw other than 0 / k");
            return LLMI_EUNSUPPORTED;
        }
        LLMI_REQUIRE(a.k > 0 && a.k % 128 == 0, "gemv: int4 weights need k a positive multiple of the 128-column group");
    }
    LLMI_REQUIRE(a.k > 0 && a.k % epl == 0, "gemv: k must be a positive multiple of 16 bytes of weights");
    LLMI_REQUIRE((size_t)a.k * 4 <= 150 * 1024, "gemv: k too large for LDS staging");
    LLMI_REQUIRE(a.w && (a.x || a.x_fixed) && (a.y || a.epi == EPI_ATOMIC), "gemv: null pointer");
    LLMI_REQUIRE(a.w_dtype != LLMI_I8 || a.scales, "gemv: int8 weights need per-row scales");
    LLMI_REQUIRE(a.w_dtype != LLMI_I4 || a.scales, "gemv: int4 weights need per-group scales");
    LLMI_REQUIRE(a.epi != EPI_ADD || a.resid, "gemv: EPI_ADD needs resid");
    LLMI_REQUIRE(a.epi != EPI_ARGMAX || a.partials, "gemv: EPI_ARGMAX needs partials");
    LLMI_REQUIRE(a.epi != EPI_SILU_MUL || (a.pair_off > 0 && a.n_rows == 2 * a.pair_off),
                 "gemv: EPI_SILU_MUL needs n_rows == 2 * pair_off");
    LLMI_REQUIRE(a.n_rows > 0, "gemv: n_rows must be > 0");
    LLMI_REQUIRE(a.epi != EPI_ATOMIC || (a.yacc && a.x && !a.x_fixed && a.ksplit >= 1 &&
                                         a.k % (a.ksplit * epl) == 0),
                 "gemv: EPI_ATOMIC needs yacc, an fp32 x and k divisible into ksplit 16-B slices");
    LLMI_REQUIRE(a.epi == EPI_ATOMIC || a.ksplit == 1, "gemv: ksplit only with EPI_ATOMIC");
    // single producer: a second K slice would overwrite the first one's row instead of adding to it
    LLMI_REQUIRE(!a.yacc_single || (a.epi == EPI_ATOMIC && a.ksplit == 1),
                 "gemv: yacc_single needs EPI_ATOMIC with ksplit 1 (one producer per row)");
    LLMI_REQUIRE(a.kpar <= 1 || ((a.kpar == 2 || a.kpar == 4) && (a.epi == EPI_STORE || a.epi == EPI_SILU_MUL) &&
                                 a.grid == 0 && (a.k / epl) % a.kpar == 0),
                 "gemv: kpar 2 / 4 needs a store or silu epilogue, an automatic grid and k / kpar whole 16-B chunks");
    LLMI_REQUIRE(a.ldw == 0 || (a.ldw >= a.k && a.ldw % epl == 0), "gemv: ldw < k or rows not 16-B aligned");
    return LLMI_OK;
}
}  // namespace

int gemv_plan(const GemvArgs& a, int* grid, int* unroll, int* xpt) {
    LLMI_TRY(gemv_check(a));
    const int kl = (a.epi == EPI_ATOMIC) ? a.k / a.ksplit : a.k;  // x extent one workgroup stages (launch_u)
    if (grid) *grid = gemv_grid(a);
    if (unroll) *unroll = gemv_pick_unroll(epl_of(a.w_dtype), a.epi, a, gemv_groups(a));
    if (xpt) *xpt = gemv_xpt(kl / 4);
    return LLMI_OK;
}

int gemv_launch(const GemvArgs& a, hipStream_t s) {
    LLMI_TRY(gemv_check(a));
    const int grid = gemv_grid(a);
    switch (a.w_dtype) {
        case LLMI_F16: return launch_epi<__half>(a, grid, s);
        case LLMI_F32: return launch_epi<float>(a, grid, s);
        case LLMI_I8: return launch_epi<int8_t>(a, grid, s);
        case LLMI_I4: return launch_epi<i4w>(a, grid, s);
    }
    return LLMI_EINVAL;
}

}  // namespace llmi
