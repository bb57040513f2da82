// Multi-row streaming GEMV for batched decode: Y[i] = W x_i for m = 2..8 activation rows in
// ONE launch, W [n_rows, k] row-major (fp16 / fp32 / int8 + row scale), fp32 accumulate.
//
// The single-row GEMV (gemv.hip) run m times reads every weight from HBM m times. Here a
// wave loads each 16-B weight chunk once (nontemporal) and dots it against m x images staged
// in LDS, so the weight stream -- the roofline of a decode step -- is paid once for the m
// sequences of a batch.
//
// Contract: row i of the output is bitwise gemv_launch's for row i alone. gemv_body sums a
// (weight row, x) pair in one fp32 accumulator per lane over chunks lane, lane + 64, ... in
// ascending order, then wave_sum, * rstd, * scale and the epilogue; this body keeps that map
// and order per (weight row, activation row) and calls the same dot_packet / block_sum /
// wave_sum / to_fixed / argmax_key. The workgroup shape (4 waves, a row group per wave) and,
// for the argmax epilogue, the grid are gemv_launch's too, so the per-workgroup argmax keys
// match entry by entry. The unroll is free (it only sets the loads in flight).
//
// LDS: the m images take m * k * 4 bytes of the CU's 160 KiB. What fits runs as one launch at
// one workgroup per CU or more; a k too wide for m images (7B down, k = 11008: 3 images) is
// run as ceil(m / fit) launches of near-equal size, a single leftover row through gemv_launch.
#include "gemv_rows_impl.h"

namespace llmi {
namespace gemv_detail {
template <typename WT>
int rows_launch_epi(const GemvRowsArgs& p, int grid, hipStream_t s);  // gemv_rows_{f16,f32,i8}.hip
}  // namespace gemv_detail

using namespace gemv_detail;

GemvArgs gemv_rows_single(const GemvRowsArgs& p, int i) {
    GemvArgs a = p.a;
    const GemvRow& r = p.row[i];
    a.x = r.x; a.x_fixed = r.x_fixed; a.x_out = r.x_out;
    a.y = r.y; a.resid = r.resid;
    a.yacc = r.yacc; a.yacc_base = r.yacc_base; a.yacc_copy = r.yacc_copy;
    a.partials = r.partials;
    a.seed_src = r.seed_src; a.seed_dst = r.seed_dst;
    return a;
}

int gemv_rows_fit(const GemvArgs& a) {
    const int kl = (a.epi == EPI_ATOMIC && a.ksplit > 1) ? a.k / a.ksplit : a.k;
    int fit = 0;
    while (fit < kGemvRowsMax && gemv_rows_lds_bytes(kl, fit + 1) <= (size_t)LLMI_ROWS_MAX_LDS) ++fit;
    return fit;
}

namespace {
int rows_launch_some(const GemvRowsArgs& p, int i0, int n, hipStream_t s) {
    if (n == 1) return gemv_launch(gemv_rows_single(p, i0), s);
    GemvRowsArgs q;
    q.a = p.a;
    q.m = n;
    for (int i = 0; i < n; ++i) q.row[i] = p.row[i0 + i];
    const int grid = gemv_grid(q.a);
    switch (q.a.w_dtype) {
        case LLMI_F16: return rows_launch_epi<__half>(q, grid, s);
        case LLMI_F32: return rows_launch_epi<float>(q, grid, s);
        case LLMI_I8: return rows_launch_epi<int8_t>(q, grid, s);
    }
    return LLMI_EINVAL;
}
}  // namespace

int gemv_rows_launch(const GemvRowsArgs& p, hipStream_t s) {
    LLMI_REQUIRE(p.m >= 2 && p.m <= kGemvRowsMax, "gemv_rows: m must be 2..8");
    const GemvArgs& a = p.a;
    if (a.w_dtype == LLMI_I4) return rows_unsupported("int4 weights are a single-row form");
    if (a.kpar > 1) return rows_unsupported("kpar > 1 is a single-row form");
    if (a.y_tag != nullptr) return rows_unsupported("granule rows are a single-row form");
    if (a.xt.buf != nullptr) return rows_unsupported("a fused exchange tail is a single-row form");
    if (a.stamps != nullptr) return rows_unsupported("no workgroup stamps");
    const bool fixed = p.row[0].x_fixed != nullptr;
    for (int i = 0; i < p.m; ++i) {
        LLMI_REQUIRE((p.row[i].x_fixed != nullptr) == fixed, "gemv_rows: the rows mix fp32 and fixed-point x");
        LLMI_REQUIRE(!p.row[i].seed_dst || !a.seed_keep || p.row[i].seed_src, "gemv_rows: seed_dst without seed_src");
        LLMI_TRY(gemv_plan(gemv_rows_single(p, i), nullptr, nullptr, nullptr));  // gemv_launch's argument contract
    }
    if (fixed ? (a.gamma == nullptr || (a.epi != EPI_STORE && a.epi != EPI_SILU_MUL && a.epi != EPI_ARGMAX))
              : (a.gamma != nullptr))
        return rows_unsupported("x is either fp32 without rmsnorm, or fixed point with rmsnorm and a store / silu / "
                                "argmax epilogue");
    const int fit = gemv_rows_fit(a);
    LLMI_REQUIRE(fit >= 1, "gemv_rows: k too large for LDS staging");
    const int parts = (p.m + fit - 1) / fit;
    for (int q = 0, i0 = 0; q < parts; ++q) {  // near-equal parts: 8 rows at fit 3 run as 3 + 3 + 2
        const int n = (p.m - i0 + (parts - q) - 1) / (parts - q);
        LLMI_TRY(rows_launch_some(p, i0, n, s));
        i0 += n;
    }
    return LLMI_OK;
}

}  // namespace llmi
