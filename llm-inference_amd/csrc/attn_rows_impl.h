// Multi-row decode attention and merge + o_proj bodies (attn_rows.hip has the design notes).
//
// Both bodies are attn_body / oproj_body (attn_impl.h) with a loop over the query rows around
// the per-row arithmetic and the loads that do not depend on the row -- the chunk's K / V rows,
// the W_o slice -- hoisted out of it. Per row they keep attn_body's / oproj_body's expressions:
// the same rotation, the same fmaf chains in the same order, the same row16_sum / wave_max /
// wave_sum / expf, the same merge order, the same to_fixed.
#pragma once
#include "attn_impl.h"

namespace llmi {
namespace attn_detail {

// LDS carve of the multi-row attention body: q, the rows' current k and v, scores, the
// per-group o partials, (m, l)
constexpr size_t kAttnRowsLds =
    (D + 2 * kAttnRowsMax * D + CH + (kThreads / LPR) * D + 4) * sizeof(float);

// One (head h, split) workgroup for the p.m query rows at positions pos0 .. pos0 + m - 1.
// HOST_SIZED (a.nact > 0): the grid holds the splits of the LAST row, nact_of(pos0 + m - 1);
// the K / V loads go out before the position arrives, as in attn_body.
template <typename KT, typename IO, bool HOST_SIZED>
__device__ __forceinline__ void attn_rows_body(const AttnRowsArgs& p, int h, int split, int ns, float* smem) {
    static_assert(!kQ8<KT>, "the multi-row attention takes no int8 cache");
    const AttnArgs& a = p.a;
    const int M = p.m;
    float* q_s = smem;
    float (*kcur_s)[D] = reinterpret_cast<float (*)[D]>(q_s + D);           // [kAttnRowsMax][D]
    float (*vcur_s)[D] = reinterpret_cast<float (*)[D]>(q_s + D + kAttnRowsMax * D);
    float* p_s = q_s + D + 2 * kAttnRowsMax * D;
    float (*o_red)[D] = reinterpret_cast<float (*)[D]>(p_s + CH);  // [groups][D]
    float* ml_s = p_s + CH + (kThreads / LPR) * D;

    const int group = a.heads / a.kv_heads;
    const int kvh = h / group;
    const int tid = threadIdx.x;
    const int grp = tid / LPR, l16 = tid % LPR;
    const int start = split * CH;
    KT* kc = reinterpret_cast<KT*>(a.k_cache) + (size_t)kvh * a.max_seq * D;
    KT* vc = reinterpret_cast<KT*>(a.v_cache) + (size_t)kvh * a.max_seq * D;
    const size_t qoff = (size_t)h * D;
    const size_t koff = (size_t)(a.heads + kvh) * D;
    const size_t voff = (size_t)(a.heads + a.kv_heads + kvh) * D;
    const int seed_per = (a.hidden + a.heads - 1) / a.heads;

    // the chunk's cached rows, once for every query row: branch-free, a row past max_seq loads
    // row `start`; rows at or past pos0 are loaded (valid memory) and never used
    Raw<KT> kr[NPG], vr[NPG];
    auto load_kv = [&]() {
#pragma unroll
        for (int t = 0; t < NPG; ++t) {
            const int j = start + grp + t * (kThreads / LPR);
            const int jj = j < a.max_seq ? j : start;
            kr[t] = ld_raw(kc + (size_t)jj * D + l16 * 8);
            vr[t] = ld_raw(vc + (size_t)jj * D + l16 * 8);
        }
    };
    int pos0;
    if constexpr (HOST_SIZED) {
        int z = 0;
        asm volatile("" : "+v"(z));  // a per-lane load: the K / V issue does not wait for it (attn_body)
        pos0 = a.pos_dev[z];
        load_kv();
    } else {
        pos0 = a.pos_dev ? *a.pos_dev : a.pos_host;
    }
    if (pos0 < 0 || pos0 + M > a.max_seq) return;  // host validates; guard against a stale state
    if constexpr (HOST_SIZED) {
        if ((pos0 + M - 1) / CH + 1 != a.nact) {
            if (a.err != nullptr && tid == 0 && split == 0) atomicOr(a.err, 4);
            return;
        }
    }
    if (start >= pos0 + M) return;  // no row's context reaches this chunk
    if constexpr (!HOST_SIZED) load_kv();

    const float qscale = 1.0f / sqrtf((float)D);
    // rotary (cos, sin) of dim pair i at position pos
    auto rope_of = [&](int pos, int i, float* c, float* s) {
        *c = 1.f;
        *s = 0.f;
        if (a.rope_tab) {
            const float2 cs = reinterpret_cast<const float2*>(a.rope_tab)[(size_t)pos * (D / 2) + i];
            *c = cs.x;
            *s = cs.y;
        } else if (a.rope) {
            rope_cs(pos, i, D, a.rope_base, c, s);
        }
    };

    // ---- the rows whose position lies in this chunk: rotated k and v as the cache will hold
    // them, into LDS (every later row reads them there), and into the cache by the kv head's
    // first query head
    for (int r = 0; r < M; ++r) {
        const int pr = pos0 + r;
        if (pr < start || pr >= start + CH) continue;  // uniform
        const float* krow = p.row[r].qkv + koff;
        const float* vrow = p.row[r].qkv + voff;
        if (tid < D / 2) {
            const int i = tid;
            float c, s;
            rope_of(pr, i, &c, &s);
            const float k0 = IO::ld(krow + i), k1 = IO::ld(krow + i + D / 2);
            kcur_s[r][i] = cache_round<KT>(k0 * c - k1 * s);
            kcur_s[r][i + D / 2] = cache_round<KT>(k1 * c + k0 * s);
        } else if (tid >= D && tid < 2 * D) {
            vcur_s[r][tid - D] = cache_round<KT>(IO::ld(vrow + tid - D));
        }
    }
    __syncthreads();
    if ((h % group) == 0 && tid < D) {
        for (int r = 0; r < M; ++r) {
            const int pr = pos0 + r;
            if (pr < start || pr >= start + CH) continue;
            store_cache(kc + (size_t)pr * D + tid, kcur_s[r][tid]);
            store_cache(vc + (size_t)pr * D + tid, vcur_s[r][tid]);
        }
    }

    // ---- the query rows, one after the other over the same registers
    for (int r = 0; r < M; ++r) {
        const int pos = pos0 + r;
        const int ctx = pos + 1;
        if (start >= ctx) continue;  // uniform: this row's context ends before the chunk
        const int end = min(start + CH, ctx);
        const float* qrow = p.row[r].qkv + qoff;
        if (tid < D / 2) {
            const int i = tid;
            float c, s;
            rope_of(pos, i, &c, &s);
            const float q0 = IO::ld(qrow + i), q1 = IO::ld(qrow + i + D / 2);
            q_s[i] = (q0 * c - q1 * s) * qscale;
            q_s[i + D / 2] = (q1 * c + q0 * s) * qscale;
        }
        __syncthreads();
        float qv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) qv[i] = q_s[l16 * 8 + i];

        // ---- scores (positions pos0 .. pos: this launch's rows, from LDS)
#pragma unroll
        for (int t = 0; t < NPG; ++t) {
            const int j = start + grp + t * (kThreads / LPR);
            float kv[8];
            if (j >= pos0) {
                const int jr = min(j - pos0, M - 1);  // (rows past pos are computed and dropped)
#pragma unroll
                for (int i = 0; i < 8; ++i) kv[i] = kcur_s[jr][l16 * 8 + i];
            } else {
                unpack8(kr[t], kv);
            }
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d = fmaf(qv[i], kv[i], d);
            d = row16_sum(d);
            if (l16 == 0 && j < end) p_s[j - start] = d;
        }
        __syncthreads();

        // ---- local softmax over this block's positions (wave 0)
        if (tid < kWave) {
            const int n = end - start;
            float s = tid < n ? p_s[tid] : -INFINITY;
            const float m = wave_max(s);
            const float pp = tid < n ? expf(s - m) : 0.f;
            const float l = wave_sum(pp);
            if (tid < n) p_s[tid] = pp;
            if (tid == 0) { ml_s[0] = m; ml_s[1] = l; }
        }
        __syncthreads();

        // ---- o = sum_j p_j v_j
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
        for (int t = 0; t < NPG; ++t) {
            const int j = start + grp + t * (kThreads / LPR);
            if (j >= end) break;
            float vv[8];
            if (j >= pos0) {
                const int jr = min(j - pos0, M - 1);
#pragma unroll
                for (int i = 0; i < 8; ++i) vv[i] = vcur_s[jr][l16 * 8 + i];
            } else {
                unpack8(vr[t], vv);
            }
            const float pj = p_s[j - start];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(pj, vv[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) o_red[grp][l16 * 8 + i] = acc[i];
        __syncthreads();

        float o = 0.f;
        if (tid < D) {
#pragma unroll
            for (int g = 0; g < kThreads / LPR; ++g) o += o_red[g][tid];
        }
        Ws ws = ws_carve(p.row[r].workspace, a.heads, ns);
        if (tid < D) IO::st(ws.o + ((size_t)h * ns + split) * D + tid, o);
        if (tid == 0) {
            IO::st(ws.ml + ((size_t)h * ns + split) * 2 + 0, ml_s[0]);
            IO::st(ws.ml + ((size_t)h * ns + split) * 2 + 1, ml_s[1]);
        }
        // split 0 of head h seeds the row's fixed-point residual accumulator (attn_body's forms)
        long long* xacc = p.row[r].xacc;
        if (xacc != nullptr && split == 0) {
            const float* resid = p.row[r].resid;
            const long long* resid_fixed = p.row[r].resid_fixed;
            const float rs = p.row[r].resid_scale;
            for (int i = h * seed_per + tid; i < min((h + 1) * seed_per, a.hidden); i += kThreads)
                IO::st_ll(xacc + i, rs == 0.f ? 0ll : resid_fixed ? resid_fixed[i] : to_fixed(resid[i]));
        }
        // (the next row's first barrier orders its q_s / p_s / o_red writes after these reads)
    }
}

// Workgroup (h, row chunk of 16 * NPL rows), oproj_body's grid for every weight dtype: the W_o
// slice is loaded once, then per query row the log-sum-exp merge of that row's partials over
// nact_of(pos0 + r) splits, the 16-lane dot products and one int64 atomic per output row into
// that row's xacc. (oproj_body2, the fp16 two-heads-per-workgroup form, adds fixed(y_a) +
// fixed(y_b) in one atomic: the integer sum of this form's two, so xacc is bitwise either's.)
template <typename WT, int NPL, typename IO>
__device__ __forceinline__ void oproj_rows_body(const OprojRowsArgs& p, int h, int chunk, int ns, float* smem) {
    const OprojArgs& a = p.a;
    const int M = p.m;
    float* m_s = smem;
    float* l_s = m_s + kMaxSplits;
    float& linv_s = l_s[kMaxSplits];
    float* o_s = l_s + kMaxSplits + 4;
    float (*o_red)[D] = reinterpret_cast<float (*)[D]>(o_s + D);
    float* y_s = o_s + 3 * D;
    const int tid = threadIdx.x;
    const int grp = tid / LPR, l16 = tid % LPR;
    const int row0 = chunk * 16 * NPL;
    const int d = tid % D, half = tid / D;

    W8<WT> wr[NPL];
    oproj_load_w<WT, NPL>(a, h, chunk, wr);
    const int pos0 = a.pos_dev ? *a.pos_dev : a.pos_host;
    if (pos0 < 0 || pos0 + M > a.max_seq) return;
    if (a.nact > 0 && (pos0 + M - 1) / CH + 1 != a.nact) return;  // (the attention launch raised bit 4)

    for (int r = 0; r < M; ++r) {
        const int nact = (pos0 + r) / CH + 1;
        Ws ws = ws_carve(p.row[r].workspace, a.heads, ns);
        const float* mlh = ws.ml + (size_t)h * ns * 2;
        const float* oh = ws.o + (size_t)h * ns * D + d;
        float ov[kMergeChunk];
#pragma unroll
        for (int i = 0; i < kMergeChunk; ++i) {
            const int sp = half + 2 * i;
            ov[i] = IO::ld(oh + (size_t)(sp < nact ? sp : 0) * D);
        }
        for (int sp = tid; sp < nact; sp += kThreads) {
            m_s[sp] = IO::ld(mlh + 2 * sp);
            l_s[sp] = IO::ld(mlh + 2 * sp + 1);
        }
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
            O = fmaf(sp < nact ? ov[i] : 0.f, sp < nact ? m_s[sp] : 0.f, O);
        }
        for (int sp = half + 2 * kMergeChunk; sp < nact; sp += 2) O = fmaf(IO::ld(oh + (size_t)sp * D), m_s[sp], O);
        o_red[half][d] = O;
        __syncthreads();
        if (tid < D) o_s[tid] = (o_red[0][tid] + o_red[1][tid]) * linv_s;
        __syncthreads();

        if constexpr (sizeof(WT) == 1 && NPL >= 2) {
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
                atomicAdd(reinterpret_cast<unsigned long long*>(p.row[r].xacc + row), (unsigned long long)to_fixed(v));
            }
        }
        // (y_s is next written after three barriers of the next row; m_s / l_s after none: order them)
        __syncthreads();
    }
}

}  // namespace attn_detail
}  // namespace llmi
