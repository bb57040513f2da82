// Multi-row decode attention + o_proj: m = 2..8 query rows of ONE sequence at consecutive
// positions p .. p + m - 1 in one attention launch and one o_proj launch (the verify step of
// speculative decoding, engine_spec.hip; llmi_debug_attn_oproj_rows).
//
// m single-row launches stream the layer's K / V cache and W_o m times. Here the grids are the
// single-row kernels' (attention: (head, split) with 64 positions a split, sized for the LAST
// row; o_proj: (head, chunk of 16 * NPL rows)), a workgroup loads its 64 K rows and 64 V rows,
// or its W_o slice, once into registers, and then loops over the query rows. The rows differ
// only in how far they see: row i's context ends at p + i, so a row leaves no partial in a
// chunk that starts past its position, and its merge runs over nact_of(p + i) splits.
//
// Positions p .. p + m - 1 are written to the cache BY this launch (the workgroup whose chunk
// owns the position, first query head of the kv head), so no workgroup may read them from the
// cache: every workgroup whose chunk holds such a position rotates and rounds those rows' k and
// v itself (cache_round<KT>: the bits a later step reads back) into LDS and takes them from
// there, exactly as the single-row kernel treats its own position.
//
// Contract: row i's partials, cache row and xacc are bitwise those of attn_decode_launch +
// attn_oproj_launch for row i alone at position p + i, the rows run in order. The per-row
// arithmetic is attn_body's / oproj_body's, expression for expression (attn_rows_impl.h); the
// residual sum is int64 fixed point, so the o_proj grid (one head a workgroup here, two in the
// fp16 single-row form) does not show in xacc.
#include "attn_rows_impl.h"

namespace llmi {
namespace {

using namespace attn_detail;

template <typename KT, bool HOST_SIZED>
__global__ __launch_bounds__(kThreads) void attn_rows_kernel(AttnRowsArgs p, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    attn_rows_body<KT, PlainIO, HOST_SIZED>(p, blockIdx.x, blockIdx.y, ns, smem);
}

template <typename WT, int NPL>
__global__ __launch_bounds__(kThreads) void oproj_rows_kernel(OprojRowsArgs p, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    oproj_rows_body<WT, NPL, PlainIO>(p, blockIdx.x, blockIdx.y, ns, smem);
}

int rows_unsupported(const char* what) {
    set_last_error(std::string("[llmi][ERROR] attn_rows: ") + what);
    return LLMI_EUNSUPPORTED;
}

template <typename WT>
int oproj_rows_launch_w(const OprojRowsArgs& p, hipStream_t s) {
    const OprojArgs& a = p.a;
    const int ns = (a.max_seq + CH - 1) / CH;
    const long target = (long)a.heads * a.n_rows / (1024 * 16);  // ~1024 workgroups (attn.hip oproj_npl)
    const int npl = target >= 8 ? 8 : target >= 4 ? 4 : target >= 2 ? 2 : 1;
    const dim3 grid(a.heads, (a.n_rows + 16 * npl - 1) / (16 * npl));
    switch (npl) {
        case 8: hipLaunchKernelGGL((oproj_rows_kernel<WT, 8>), grid, dim3(kThreads), oproj_lds<8>(), s, p, ns); break;
        case 4: hipLaunchKernelGGL((oproj_rows_kernel<WT, 4>), grid, dim3(kThreads), oproj_lds<4>(), s, p, ns); break;
        case 2: hipLaunchKernelGGL((oproj_rows_kernel<WT, 2>), grid, dim3(kThreads), oproj_lds<2>(), s, p, ns); break;
        default: hipLaunchKernelGGL((oproj_rows_kernel<WT, 1>), grid, dim3(kThreads), oproj_lds<1>(), s, p, ns); break;
    }
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace

int attn_rows_launch(const AttnRowsArgs& p, hipStream_t s) {
    const AttnArgs& a = p.a;
    LLMI_REQUIRE(p.m >= 2 && p.m <= kAttnRowsMax, "attn_rows: m must be 2..8");
    if (a.cache_dtype == LLMI_I8) return rows_unsupported("an int8 cache is a single-row form");
    if (a.direct_out) return rows_unsupported("the merged output (direct_out) is a single-row form");
    if (a.qkv_tag != nullptr || a.publish) return rows_unsupported("granule rows are a single-row form");
    if (a.stamps != nullptr) return rows_unsupported("no workgroup stamps");
    LLMI_REQUIRE(a.head_dim == D, "attn_rows: head_dim must be 128");
    LLMI_REQUIRE(a.heads > 0 && a.kv_heads > 0 && a.heads % a.kv_heads == 0, "attn_rows: bad head counts");
    LLMI_REQUIRE(a.max_seq > 0 && (a.max_seq + CH - 1) / CH <= kMaxSplits, "attn_rows: max_seq out of range");
    LLMI_REQUIRE(a.cache_dtype == LLMI_F16 || a.cache_dtype == LLMI_F32, "attn_rows: cache dtype must be f16 or f32");
    LLMI_REQUIRE(a.pos_dev || (a.pos_host >= 0 && a.pos_host + p.m <= a.max_seq), "attn_rows: positions out of range");
    LLMI_REQUIRE(a.k_cache && a.v_cache, "attn_rows: null cache");
    const int ns = (a.max_seq + CH - 1) / CH;
    LLMI_REQUIRE(a.nact >= 0 && a.nact <= ns, "attn_rows: nact out of range");
    LLMI_REQUIRE(a.nact == 0 || a.pos_dev, "attn_rows: nact > 0 needs the device position");
    for (int i = 0; i < p.m; ++i) {
        const AttnRow& r = p.row[i];
        LLMI_REQUIRE(r.qkv && r.workspace, "attn_rows: a row's qkv or workspace is null");
        LLMI_REQUIRE(!r.xacc || r.resid || r.resid_fixed, "attn_rows: xacc seeding needs resid");
    }
    const bool hs = a.nact > 0;
    const dim3 grid(a.heads, hs ? a.nact : ns);
    if (a.cache_dtype == LLMI_F16) {
        if (hs)
            hipLaunchKernelGGL((attn_rows_kernel<__half, true>), grid, dim3(kThreads), kAttnRowsLds, s, p, ns);
        else
            hipLaunchKernelGGL((attn_rows_kernel<__half, false>), grid, dim3(kThreads), kAttnRowsLds, s, p, ns);
    } else {
        if (hs)
            hipLaunchKernelGGL((attn_rows_kernel<float, true>), grid, dim3(kThreads), kAttnRowsLds, s, p, ns);
        else
            hipLaunchKernelGGL((attn_rows_kernel<float, false>), grid, dim3(kThreads), kAttnRowsLds, s, p, ns);
    }
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int oproj_rows_launch(const OprojRowsArgs& p, hipStream_t s) {
    const OprojArgs& a = p.a;
    LLMI_REQUIRE(p.m >= 2 && p.m <= kAttnRowsMax, "oproj_rows: m must be 2..8");
    if (a.xt.buf != nullptr) return rows_unsupported("a fused exchange tail is a single-row form");
    if (a.stamps != nullptr) return rows_unsupported("no workgroup stamps");
    LLMI_REQUIRE(a.head_dim == D, "oproj_rows: head_dim must be 128");
    LLMI_REQUIRE(a.w && a.heads > 0 && a.n_rows > 0, "oproj_rows: bad arguments");
    LLMI_REQUIRE(a.ldw >= a.heads * D, "oproj_rows: ldw < heads * head_dim");
    LLMI_REQUIRE(a.ldw % 16 == 0, "oproj_rows: ldw must be a multiple of 16 elements (16-B row slices)");
    LLMI_REQUIRE(a.max_seq > 0 && (a.max_seq + CH - 1) / CH <= kMaxSplits, "oproj_rows: max_seq out of range");
    LLMI_REQUIRE(a.nact >= 0 && a.nact <= (a.max_seq + CH - 1) / CH, "oproj_rows: nact out of range");
    LLMI_REQUIRE(a.pos_dev || (a.pos_host >= 0 && a.pos_host + p.m <= a.max_seq), "oproj_rows: positions out of range");
    for (int i = 0; i < p.m; ++i)
        LLMI_REQUIRE(p.row[i].workspace && p.row[i].xacc, "oproj_rows: a row's workspace or xacc is null");
    switch (a.w_dtype) {
        case LLMI_F16: return oproj_rows_launch_w<__half>(p, s);
        case LLMI_F32: return oproj_rows_launch_w<float>(p, s);
        case LLMI_I8:
            LLMI_REQUIRE(a.scales != nullptr, "oproj_rows: int8 weights need scales");
            return oproj_rows_launch_w<int8_t>(p, s);
    }
    LLMI_REQUIRE(false, "oproj_rows: weight dtype must be f16, f32 or i8");
}

}  // namespace llmi
