// Batched decode attention + o_proj: the active slots of a Batch (engine_batch.hip, option
// "batch_attn"; llmi_debug_attn_oproj_batch) in ONE attention launch and ONE o_proj launch a
// layer instead of one pair per slot.
//
// The slots are unrelated sequences: each has its own cache, position, split count, workspace,
// xacc and error word, so nothing of attn_rows.hip's sharing (one cache, consecutive positions)
// applies. What they share is W_o -- 33.5 MB a 7B layer, streamed once per slot by the per-slot
// launches -- and the launch itself: at batch contexts a slot's attention grid is a few dozen
// workgroups on 256 CUs, its cost the launch, not the work.
//
// attn_batch_kernel: grid (heads, max over the slots of nact, slots). blockIdx.z picks the slot's
// record out of the kernel arguments (held by value, as GemvRowsArgs holds its rows: scalar loads
// from the argument segment, no pointer table in memory); a workgroup whose split is at or past
// its slot's split count leaves before it issues a load; every other workgroup is attn_body's
// host-sized form on that slot's arguments -- the same function, so the slot's cache row,
// partials, xacc seed and error bit are the single-sequence launch's.
//
// oproj_batch_kernel: oproj_body's grid for every weight dtype, (head, chunk of 16 * NPL rows).
// A workgroup issues its W_o slice first and keeps it in registers for the whole launch (NPL
// 16-B loads a lane), then walks the slots: merge of that slot's partials over that slot's live
// splits (no load for a split >= nact), the 16-lane dot products, one int64 atomic per output row
// into that slot's xacc. The walk is software-pipelined: a slot's merge is five workgroup
// barriers behind one load round trip, and eight of those in series would cost more than the W_o
// stream they sit behind, so the partial and (m, l) loads of slot r + 1 are issued into a second
// register set before slot r's first barrier and land while slot r merges and multiplies.
//
// Contract: slot s's xacc is the integer sum of the same to_fixed(y) terms attn_oproj_launch adds
// (the merge order, fmaf chains, row16_sum / oct8_sum and scales are oproj_body's), so it is
// bitwise the single-sequence pair's and depends on no other slot.
#include "attn_impl.h"

namespace llmi {
namespace {

using namespace attn_detail;

template <typename KT>
__global__ __launch_bounds__(kThreads) void attn_batch_kernel(AttnBatchArgs p, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AttnBatchSlot& sl = p.slot[blockIdx.z];
    if ((int)blockIdx.y >= sl.nact) return;  // this slot's context ends before the split
    AttnArgs a = p.a;
    a.qkv = sl.qkv;
    a.k_cache = sl.k_cache; a.v_cache = sl.v_cache;
    a.k_scale = sl.k_scale; a.v_scale = sl.v_scale;
    a.pos_dev = sl.pos_dev; a.nact = sl.nact;
    a.workspace = sl.workspace;
    a.xacc = sl.xacc; a.resid = sl.resid; a.resid_fixed = sl.resid_fixed; a.resid_scale = sl.resid_scale;
    a.err = sl.err;
    attn_body<KT, PlainIO, true>(a, blockIdx.x, blockIdx.y, ns, smem);
}

// one slot's partials of head h as a thread holds them between issue and use: the o values of
// its dim for splits half + 2 i (i < kMergeChunk), and (m, l) of splits tid + i * kThreads
constexpr int kMlPer = kMaxSplits / kThreads;
struct Partials {
    float ov[kMergeChunk];
    float2 ml[kMlPer];
};
// Issue the loads, none for a split at or past nact. Every guard is uniform over a wave (half is:
// D = two waves), so a dead split costs a scalar compare, not a predicated load.
__device__ __forceinline__ void ld_partials(const AttnBatchSlot& sl, int heads, int h, int ns, Partials& q) {
    const int tid = threadIdx.x;
    const int d = tid % D, half = tid / D;
    const int nact = min(sl.nact, ns);
    Ws ws = ws_carve(sl.workspace, heads, ns);
    const float* mlh = ws.ml + (size_t)h * ns * 2;
    const float* oh = ws.o + (size_t)h * ns * D + d;
#pragma unroll
    for (int i = 0; i < kMergeChunk; ++i) {
        const int sp = half + 2 * i;
        q.ov[i] = 0.f;
        if (sp < nact) q.ov[i] = PlainIO::ld(oh + (size_t)sp * D);
    }
#pragma unroll
    for (int i = 0; i < kMlPer; ++i) {
        if (i * kThreads < nact) {
            const int sp = min(tid + i * kThreads, nact - 1);
            q.ml[i] = PlainIO::ld2(reinterpret_cast<const float2*>(mlh + 2 * sp));
        }
    }
}

template <typename WT, int NPL>
__global__ __launch_bounds__(kThreads) void oproj_batch_kernel(OprojBatchArgs p, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const OprojArgs& a = p.a;
    float* m_s = smem;
    float* l_s = m_s + kMaxSplits;
    float& linv_s = l_s[kMaxSplits];
    float* o_s = l_s + kMaxSplits + 4;
    float (*o_red)[D] = reinterpret_cast<float (*)[D]>(o_s + D);
    float* y_s = o_s + 3 * D;
    const int h = blockIdx.x, chunk = blockIdx.y;
    const int tid = threadIdx.x;
    const int grp = tid / LPR, l16 = tid % LPR;
    const int row0 = chunk * 16 * NPL;
    const int d = tid % D, half = tid / D;

    W8<WT> wr[NPL];
    oproj_load_w<WT, NPL>(a, h, chunk, wr);
    Partials cur, nxt;
    ld_partials(p.slot[0], a.heads, h, ns, cur);

    for (int r = 0; r < p.n; ++r) {
        const AttnBatchSlot& sl = p.slot[r];
        const int nact = min(sl.nact, ns);
#pragma unroll
        for (int i = 0; i < kMlPer; ++i) {
            const int sp = tid + i * kThreads;
            if (i * kThreads < nact && sp < nact) {
                m_s[sp] = cur.ml[i].x;
                l_s[sp] = cur.ml[i].y;
            }
        }
        // the next slot's partials: in flight across this slot's barriers and dot products
        if (r + 1 < p.n) ld_partials(p.slot[r + 1], a.heads, h, ns, nxt);
        __syncthreads();
        // log-sum-exp weights by wave 0 (one expf per split), into LDS
        if (tid < kWave) {
            float Mx = -INFINITY;
            for (int sp = tid; sp < nact; sp += kWave) Mx = fmaxf(Mx, m_s[sp]);
            Mx = wave_max(Mx);
            float lsum = 0.f;
            for (int sp = tid; sp < nact; sp += kWave) {
                const float wgt = expf(m_s[sp] - Mx);
                m_s[sp] = wgt;
                lsum = fmaf(l_s[sp], wgt, lsum);
            }
            lsum = wave_sum(lsum);
            if (tid == 0) linv_s = 1.0f / lsum;
        }
        __syncthreads();
        float O = 0.f;
#pragma unroll
        for (int i = 0; i < kMergeChunk; ++i) {
            const int sp = half + 2 * i;
            O = fmaf(sp < nact ? cur.ov[i] : 0.f, sp < nact ? m_s[sp] : 0.f, O);
        }
        if (nact > 2 * kMergeChunk) {  // past ctx 2048: the further splits straight from memory
            const float* oh = ws_carve(sl.workspace, a.heads, ns).o + (size_t)h * ns * D + d;
            for (int sp = half + 2 * kMergeChunk; sp < nact; sp += 2)
                O = fmaf(PlainIO::ld(oh + (size_t)sp * D), m_s[sp], O);
        }
        o_red[half][d] = O;
        __syncthreads();
        if (tid < D) o_s[tid] = (o_red[0][tid] + o_red[1][tid]) * linv_s;
        __syncthreads();

        if constexpr (sizeof(WT) == 1 && NPL >= 2) {
            // int8: 8 lanes a row, two rows a 16-lane group (oproj_load_w's map)
            float x16[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) x16[i] = o_s[(l16 & 7) * 16 + i];
#pragma unroll
            for (int u = 0; u < NPL / 2; ++u) {
                const uint32_t q[4] = {wr[u].v[0].x, wr[u].v[0].y, wr[u].v[0].z, wr[u].v[0].w};
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    acc = fmaf((float)(int8_t)((q[i / 4] >> (8 * (i % 4))) & 0xff), x16[i], acc);
                acc = oct8_sum(acc);
                if ((l16 & 7) == 0) y_s[grp + 16 * (2 * u + (l16 >> 3))] = acc;
            }
        } else {
            float xv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) xv[i] = o_s[l16 * 8 + i];
#pragma unroll
            for (int t = 0; t < NPL; ++t) {
                float wv[8];
                unpack_w8<WT>(wr[t], wv);
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc = fmaf(wv[i], xv[i], acc);
                acc = row16_sum(acc);
                if (l16 == 0) y_s[grp + 16 * t] = acc;
            }
        }
        __syncthreads();
        if (tid < 16 * NPL) {
            const int row = row0 + tid;
            if (row < a.n_rows) {
                float v = y_s[tid];
                if (a.scales) v *= __half2float(a.scales[row]);
                atomicAdd(reinterpret_cast<unsigned long long*>(sl.xacc + row), (unsigned long long)to_fixed(v));
            }
        }
        // (no barrier here: every LDS array this slot read is next written behind at least two of
        // the next slot's barriers -- m_s / l_s were last read before this slot's third)
        if (r + 1 < p.n) cur = nxt;
    }
}

int batch_unsupported(const char* what) {
    set_last_error(std::string("[llmi][ERROR] attn_batch: ") + what);
    return LLMI_EUNSUPPORTED;
}

template <typename KT>
void attn_batch_launch_k(const AttnBatchArgs& p, dim3 grid, int ns, hipStream_t s) {
    hipLaunchKernelGGL((attn_batch_kernel<KT>), grid, dim3(kThreads), kAttnLds, s, p, ns);
}

template <typename WT>
int oproj_batch_launch_w(const OprojBatchArgs& p, hipStream_t s) {
    const OprojArgs& a = p.a;
    const int ns = (a.max_seq + CH - 1) / CH;
    const long target = (long)a.heads * a.n_rows / (1024 * 16);  // ~1024 workgroups (attn.hip oproj_npl)
    const int npl = target >= 8 ? 8 : target >= 4 ? 4 : target >= 2 ? 2 : 1;
    const dim3 grid(a.heads, (a.n_rows + 16 * npl - 1) / (16 * npl));
    switch (npl) {
        case 8: hipLaunchKernelGGL((oproj_batch_kernel<WT, 8>), grid, dim3(kThreads), oproj_lds<8>(), s, p, ns); break;
        case 4: hipLaunchKernelGGL((oproj_batch_kernel<WT, 4>), grid, dim3(kThreads), oproj_lds<4>(), s, p, ns); break;
        case 2: hipLaunchKernelGGL((oproj_batch_kernel<WT, 2>), grid, dim3(kThreads), oproj_lds<2>(), s, p, ns); break;
        default: hipLaunchKernelGGL((oproj_batch_kernel<WT, 1>), grid, dim3(kThreads), oproj_lds<1>(), s, p, ns); break;
    }
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace

int attn_batch_launch(const AttnBatchArgs& p, hipStream_t s) {
    const AttnArgs& a = p.a;
    LLMI_REQUIRE(p.n >= 1 && p.n <= kAttnBatchMax, "attn_batch: n must be 1..8");
    if (a.direct_out) return batch_unsupported("the merged output (direct_out) is a single-sequence form");
    if (a.qkv_tag != nullptr || a.publish) return batch_unsupported("granule rows are a single-sequence form");
    if (a.stamps != nullptr) return batch_unsupported("no workgroup stamps");
    LLMI_REQUIRE(a.head_dim == D, "attn_batch: head_dim must be 128");
    LLMI_REQUIRE(a.heads > 0 && a.kv_heads > 0 && a.heads % a.kv_heads == 0, "attn_batch: bad head counts");
    LLMI_REQUIRE(a.max_seq > 0 && (a.max_seq + CH - 1) / CH <= kMaxSplits, "attn_batch: max_seq out of range");
    LLMI_REQUIRE(a.cache_dtype == LLMI_F16 || a.cache_dtype == LLMI_F32 || a.cache_dtype == LLMI_I8,
                 "attn_batch: cache dtype must be f16, f32 or i8");
    const int ns = (a.max_seq + CH - 1) / CH;
    int top = 0;
    for (int i = 0; i < p.n; ++i) {
        const AttnBatchSlot& r = p.slot[i];
        LLMI_REQUIRE(r.qkv && r.k_cache && r.v_cache && r.workspace, "attn_batch: a slot's qkv, cache or workspace is null");
        LLMI_REQUIRE(r.pos_dev && r.nact > 0 && r.nact <= ns,
                     "attn_batch: every slot needs its device position and its host-sized nact (1..max_seq / 64)");
        LLMI_REQUIRE(!r.xacc || r.resid || r.resid_fixed, "attn_batch: xacc seeding needs resid");
        if (a.cache_dtype == LLMI_I8) {
            LLMI_REQUIRE(r.k_scale && r.v_scale, "attn_batch: an int8 cache needs its row scales (k_scale, v_scale)");
            LLMI_REQUIRE((uintptr_t)r.k_cache % 8 == 0 && (uintptr_t)r.v_cache % 8 == 0 &&
                             (uintptr_t)r.k_scale % 2 == 0 && (uintptr_t)r.v_scale % 2 == 0,
                         "attn_batch: an int8 cache must be 8-byte aligned, its scales 2-byte");
        }
        top = r.nact > top ? r.nact : top;
    }
    const dim3 grid(a.heads, top, p.n);
    switch (a.cache_dtype) {
        case LLMI_F16: attn_batch_launch_k<__half>(p, grid, ns, s); break;
        case LLMI_F32: attn_batch_launch_k<float>(p, grid, ns, s); break;
        default: attn_batch_launch_k<int8_t>(p, grid, ns, s); break;
    }
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int oproj_batch_launch(const OprojBatchArgs& p, hipStream_t s) {
    const OprojArgs& a = p.a;
    LLMI_REQUIRE(p.n >= 1 && p.n <= kAttnBatchMax, "oproj_batch: n must be 1..8");
    if (a.xt.buf != nullptr) return batch_unsupported("a fused exchange tail is a single-sequence form");
    if (a.stamps != nullptr) return batch_unsupported("no workgroup stamps");
    LLMI_REQUIRE(a.head_dim == D, "oproj_batch: head_dim must be 128");
    LLMI_REQUIRE(a.w && a.heads > 0 && a.n_rows > 0, "oproj_batch: bad arguments");
    LLMI_REQUIRE(a.ldw >= a.heads * D, "oproj_batch: ldw < heads * head_dim");
    LLMI_REQUIRE(a.ldw % 16 == 0, "oproj_batch: ldw must be a multiple of 16 elements (16-B row slices)");
    LLMI_REQUIRE(a.max_seq > 0 && (a.max_seq + CH - 1) / CH <= kMaxSplits, "oproj_batch: max_seq out of range");
    for (int i = 0; i < p.n; ++i) {
        const AttnBatchSlot& r = p.slot[i];
        LLMI_REQUIRE(r.workspace && r.xacc, "oproj_batch: a slot's workspace or xacc is null");
        LLMI_REQUIRE(r.nact > 0 && r.nact <= (a.max_seq + CH - 1) / CH, "oproj_batch: a slot's nact out of range");
    }
    switch (a.w_dtype) {
        case LLMI_F16: return oproj_batch_launch_w<__half>(p, s);
        case LLMI_F32: return oproj_batch_launch_w<float>(p, s);
        case LLMI_I8:
            LLMI_REQUIRE(a.scales != nullptr, "oproj_batch: int8 weights need scales");
            return oproj_batch_launch_w<int8_t>(p, s);
    }
    LLMI_REQUIRE(false, "oproj_batch: weight dtype must be f16, f32 or i8");
}

}  // namespace llmi
