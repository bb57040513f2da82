// Grouped-query decode attention on the matrix cores (opt-in: AttnArgs::gqa, engine / batch option
// "gqa_attn"; DESIGN.md §3 "Grouped-query decode attention"). attn_body (attn_impl.h) runs one
// workgroup per QUERY head and split, so with heads / kv_heads = g every cached K and V row is
// requested g times. Here one workgroup is one (KV head, 64-position split): it loads its 64 K rows
// and 64 V rows once and serves the g <= 8 query heads of that kv head. Same AttnArgs, same
// per-(query head, split) partials (O[128], m, l) in the same workspace, same cache write, xacc
// seed and error bits as attn_body: attn_oproj_launch / the merge run unchanged after it. Faithful
// to fp32 (4e-6 operator bar), not bitwise attn_body's. No inter-workgroup waits: a plain grid.
//
// Scores, S[j][h] = sum_d K[j][d] q_h[d]: v_mfma_f32_16x16x32_f16 with a 16-position x 32-dim K
// tile as A and the group's rotated q rows as B in two fp16 planes -- column h is hi = fp16(q_h),
// column 8 + h is lo = fp16(q_h - hi), unused columns zero; column 8 + h of the fp32 tile is added
// to column h (one DPP row rotation). Wave w owns positions 16 w .. 16 w + 15: lane (r = lane % 16,
// c = lane / 16) loads the 16-byte chunks 4 s + c of row 16 w + r (fp16: s < 4, 8 dims each; int8:
// s < 2, 16 dims each, converted exactly in registers to two operands), and the chunk IS its A
// operand (global -> VGPR -> MFMA, as gemv_rows_mfma.hip); B is built from the fp32 q image in LDS
// with the same (s, c) -> dims map. Then * s_k[j] (int8: the row scale stays outside the product),
// * 1/sqrt(d), and the fp32 softmax of attn_body over the split's positions, one wave per head.
//
// P V, O^T[d][h] = sum_j V[j][d] p_h[j]: A is a 16-dim x 32-position tile of V^T, B the 32
// positions of p in two fp16 planes. V's rows are contiguous in d, the MFMA wants 8 positions of
// one d per lane, so V goes through LDS: a row-major fp16 image [64][128 + 16] written with the
// 16-byte chunks as loaded (int8 converted, exact) and read back as 8 two-byte loads per operand.
// The k slot 8 c + i of a step holds position c + 4 i, so the four c of one load are adjacent
// image rows: with the 288-byte row stride (72 words) lane (r, c) reads bank 8 c + r / 2, 32
// distinct banks -- the padded layout, chosen over ds_read_b64_tr_b16 because the image is read
// once (4 MFMAs a wave): the transposed read would save 28 LDS instructions a lane and fix the
// lane -> row map to the hardware's, where this map is free to follow the loads. p is stored at its
// slot, so the B operand is one 16-byte LDS read. Before the planes are formed p_j (int8:
// p_j * s_v[j]) is scaled by the power of two that puts the head's largest weight in [2^13, 2^14):
// weights down to 2^-28 of the largest stay normal fp16 numbers in both planes (unscaled, an int8
// row's p s_v ~ 1e-4 would sit in the subnormals and lose the lo plane); the fp32 tile is scaled
// back exactly. Wave w owns dims 32 w .. 32 w + 31 of all heads (2 tiles x 2 steps).
//
// Stale rows (positions >= pos, int8: their scales) are loaded -- the host-sized form issues every
// load before the position arrives -- and replaced by zeros through selects before any product;
// the current position's k and v come from LDS (rounded as the cache holds them: cache_round,
// q8_round_row), never from the cache. Every sum has a fixed order: the MFMA's, wave_max / wave_sum.
//
// LDS 28,016 B (q 4 KiB, current k/v 1 KiB, scores 2 KiB, V image 18 KiB, p planes 2.25 KiB);
// hipcc remarks (gfx950): 78 / 76 VGPRs (fp16 cache, host-sized / max_seq-sized grid), 64 / 68 (int8),
// no scratch, no spills, occupancy 5 waves a SIMD (five workgroups a CU: the LDS bound).
#include "attn_impl.h"

namespace llmi {
namespace {

using namespace attn_detail;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kP = 64;       // positions of a workgroup: the split of the workspace (CH)
constexpr int kG = 8;        // query heads of a kv head at most (two planes: 16 MFMA columns)
constexpr int kVS = D + 16;  // halves of a V image row: 72 words, see above
constexpr int kPS = kP + 8;  // halves of a p plane row

struct Lds {
    float q[kG][D];        // rotated q rows of the group (fp32, unscaled)
    float kcur[D], vcur[D];  // the current position's k and v as the cache holds them
    float s[kG][kP];       // scores
    alignas(16) _Float16 v[kP][kVS];
    alignas(16) _Float16 p[2 * kG][kPS];  // [plane * 8 + head][k slot]
    float ml[kG][2];
    float pinv[kG];        // 2^-e of the head's planes
    float cur_sc[2];       // int8: scales of the current k and v rows
};

// 8 int8 -> 8 fp16, exact (gemv_rows_mfma.hip): byte b ^ 0x80 under the exponent byte of fp16 1024
__device__ __forceinline__ h8 i8x8_to_h8(uint32_t w0, uint32_t w1) {
    const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
    const uint32_t x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
    const h2 r0 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04010400u)) - bias;
    const h2 r1 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04030402u)) - bias;
    const h2 r2 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04010400u)) - bias;
    const h2 r3 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04030402u)) - bias;
    return (h8){r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
}
// 8 floats of LDS that fp16 holds exactly (cache_round's values, q8_round_row's integers)
__device__ __forceinline__ h8 f8_to_h8(const float* p) {
    h8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (_Float16)p[i];
    return r;
}

// workgroup (kv head, split); ns: the workspace's split stride; the grid holds ns splits, or only
// the a.nact active ones (HOST_SIZED: every load that needs no position is issued before it arrives)
template <typename KT, bool HOST_SIZED>
__global__ __launch_bounds__(kThreads) void attn_gqa_kernel(AttnArgs a, int ns) {
    constexpr bool Q8 = kQ8<KT>;
    constexpr int NK = Q8 ? 2 : 4;   // 16-byte chunks of a row per lane
    constexpr int CD = Q8 ? 16 : 8;  // dims of a chunk
    __shared__ Lds sm;
    WgStamp ts(a.stamps);
    const int kvh = blockIdx.x, split = blockIdx.y;
    const int group = a.heads / a.kv_heads, h0 = kvh * group;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, c4 = lane >> 4;
    const int start = split * kP;
    const int jrow = start + 16 * wave + r16;  // the cached row whose chunks this lane loads
    KT* kc = reinterpret_cast<KT*>(a.k_cache) + (size_t)kvh * a.max_seq * D;
    KT* vc = reinterpret_cast<KT*>(a.v_cache) + (size_t)kvh * a.max_seq * D;
    __half* ksc = nullptr;
    __half* vsc = nullptr;
    if constexpr (Q8) {
        ksc = a.k_scale + (size_t)kvh * a.max_seq;
        vsc = a.v_scale + (size_t)kvh * a.max_seq;
    }
    uint4 kr[NK], vr[NK];
    __half ksr[4], vsr = __ushort_as_half(0);  // int8: scales of the C tile's rows / of row `lane`
    (void)ksr;
    // branch-free: rows past max_seq load row `start`; rows at or past the position are valid
    // cache memory and are replaced by selects below
    auto issue = [&]() {
        const int jj = jrow < a.max_seq ? jrow : start;
        const KT* kp = kc + (size_t)jj * D + c4 * CD;
        const KT* vp = vc + (size_t)jj * D + c4 * CD;
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            kr[s] = ld_nt16(kp + 4 * s * CD);
            vr[s] = ld_nt16(vp + 4 * s * CD);
        }
        if constexpr (Q8) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = start + 16 * wave + 4 * c4 + r;
                ksr[r] = ksc[j < a.max_seq ? j : start];
            }
            vsr = vsc[start + lane < a.max_seq ? start + lane : start];
        }
    };
    int pos;
    if constexpr (HOST_SIZED) {
        int z = 0;
        asm volatile("" : "+v"(z));  // a per-lane load: the position stays in a VGPR (attn_body)
        pos = a.pos_dev[z];
        issue();
    } else {
        pos = a.pos_dev ? *a.pos_dev : a.pos_host;
    }
    if (pos < 0 || pos >= a.max_seq) return;  // host validates; guard against a stale state
    if constexpr (HOST_SIZED) {
        if (pos / CH + 1 != a.nact) {  // the grid came from the host's position (attn_body)
            if (a.err != nullptr && tid == 0 && split == 0) atomicOr(a.err, 4);
            return;
        }
    }
    const int ctx = pos + 1;
    if (start >= ctx) return;
    const int end = min(start + kP, ctx);
    const int nact = (ctx + CH - 1) / CH;
    const bool owns_pos = (end == ctx);
    if constexpr (!HOST_SIZED) issue();

    // ---- RoPE of the group's q rows (waves take heads w, w + 4) and, in the split that owns the
    // position, of the current k (wave 3); the current v (waves 1, 2). attn_body's expressions.
    {
        const int i = lane;  // the pair (i, i + d/2)
        float c = 1.f, s = 0.f;
        if (a.rope_tab) {
            const float2 cs = reinterpret_cast<const float2*>(a.rope_tab)[(size_t)pos * (D / 2) + i];
            c = cs.x;
            s = cs.y;
        } else if (a.rope) {
            rope_cs(pos, i, D, a.rope_base, &c, &s);
        }
        for (int g = wave; g < group; g += kThreads / kWave) {
            const float* qrow = a.qkv + (size_t)(h0 + g) * D;
            const float q0 = qrow[i], q1 = qrow[i + D / 2];
            sm.q[g][i] = q0 * c - q1 * s;
            sm.q[g][i + D / 2] = q1 * c + q0 * s;
        }
        if (owns_pos) {
            if (wave == 3) {
                const float* krow = a.qkv + (size_t)(a.heads + kvh) * D;
                const float k0 = krow[i], k1 = krow[i + D / 2];
                sm.kcur[i] = cache_round<KT>(k0 * c - k1 * s);
                sm.kcur[i + D / 2] = cache_round<KT>(k1 * c + k0 * s);
            } else if (wave != 0) {
                const float* vrow = a.qkv + (size_t)(a.heads + a.kv_heads + kvh) * D;
                sm.vcur[tid - kWave] = cache_round<KT>(vrow[tid - kWave]);
            }
        }
    }
    __syncthreads();
    ts.mark(1);  // timeline: q rotated, this split's K/V rows in flight or in registers

    // ---- cache write at slot pos, once per kv head; the current position is always taken from LDS
    if constexpr (Q8) {
        if (owns_pos) {  // uniform; wave 0 rounds and writes the k row, wave 1 the v row
            if (wave < 2) {
                const bool isv = wave == 1;
                const unsigned short sb = q8_round_row(isv ? sm.vcur : sm.kcur, true, (isv ? vc : kc) + (size_t)pos * D,
                                                       (isv ? vsc : ksc) + pos);
                if (lane == 0) sm.cur_sc[isv ? 1 : 0] = __half2float(__ushort_as_half(sb));
            }
            __syncthreads();
        }
    } else {
        if (owns_pos && tid < D) {
            store_cache(kc + (size_t)pos * D + tid, sm.kcur[tid]);
            store_cache(vc + (size_t)pos * D + tid, sm.vcur[tid]);
        }
    }

    // ---- scores of positions 16 w .. 16 w + 15 for every head; the V image
    const int hd = r16 & 7;          // this lane's B / C column: head hd, plane lo
    const bool lo = r16 >= 8, live = hd < group;
    const bool keep = jrow < pos, cur = jrow == pos;  // a cached row of the context / the current row
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto q_frag = [&](int d0) {  // the planes' 8 dims from d0 of column r16
        h8 b;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v = live ? sm.q[hd][d0 + i] : 0.f;
            const _Float16 hi = (_Float16)v;
            b[i] = lo ? (_Float16)(v - (float)hi) : hi;
        }
        return b;
    };
    // the operand a loaded chunk half gives: zeros for a stale row, the LDS row for the current one
    auto operand = [&](h8 raw, const float* cur_row, int d0) {
        h8 v = keep ? raw : zero8;
        if (cur) v = f8_to_h8(cur_row + d0);
        return v;
    };
    _Float16* vimg = &sm.v[16 * wave + r16][0];
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const int d0 = (4 * s + c4) * CD;
        if constexpr (Q8) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(operand(i8x8_to_h8(kr[s].x, kr[s].y), sm.kcur, d0),
                                                         q_frag(d0), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(operand(i8x8_to_h8(kr[s].z, kr[s].w), sm.kcur, d0 + 8),
                                                         q_frag(d0 + 8), acc, 0, 0, 0);
            *reinterpret_cast<h8*>(vimg + d0) = operand(i8x8_to_h8(vr[s].x, vr[s].y), sm.vcur, d0);
            *reinterpret_cast<h8*>(vimg + d0 + 8) = operand(i8x8_to_h8(vr[s].z, vr[s].w), sm.vcur, d0 + 8);
        } else {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(operand(__builtin_bit_cast(h8, kr[s]), sm.kcur, d0),
                                                         q_frag(d0), acc, 0, 0, 0);
            *reinterpret_cast<h8*>(vimg + d0) = operand(__builtin_bit_cast(h8, vr[s]), sm.vcur, d0);
        }
    }
    // lane (column r16, c4) holds positions 16 w + 4 c4 + r of its column: lo + hi, the scales
    const float qscale = 1.0f / sqrtf((float)D);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jl = 16 * wave + 4 * c4 + r, j = start + jl;
        float sc = acc[r] + row_ror<8>(acc[r]);
        // int8: the row's scale after the integer sum, a select (a stale row's NaN scale is never used)
        if constexpr (Q8) sc *= (j == pos) ? sm.cur_sc[0] : (j < pos ? __half2float(ksr[r]) : 0.f);
        sc *= qscale;
        if (!lo && live) sm.s[hd][jl] = sc;
    }
    __syncthreads();

    // ---- fp32 softmax over the split's positions, a wave per head (attn_body's), and the planes of p
    {
        const int n = end - start;
        // position lane = 32 st + c + 4 i sits in k slot 32 st + 8 c + i
        const int slot = (lane & 32) + 8 * (lane & 3) + ((lane & 31) >> 2);
        for (int g = wave; g < kG; g += kThreads / kWave) {
            if (g >= group) {  // unused columns are zero
                sm.p[g][lane] = (_Float16)0.f;
                sm.p[kG + g][lane] = (_Float16)0.f;
                continue;
            }
            const float s = lane < n ? sm.s[g][lane] : -INFINITY;
            const float m = wave_max(s);
            const float p = lane < n ? expf(s - m) : 0.f;
            const float l = wave_sum(p);
            float pw = p;  // int8: s_v folded into p (a select: stale scales are NaN)
            if constexpr (Q8)
                pw = lane < n ? p * ((start + lane == pos) ? sm.cur_sc[1] : __half2float(vsr)) : 0.f;
            // 2^e with max(pw) * 2^e in [2^13, 2^14): biased exponents, exact both ways
            const int ex = (int)((__float_as_uint(wave_max(pw)) >> 23) & 0xffu);
            const int up = min(max(267 - ex, 1), 253);
            const float x = pw * __uint_as_float((unsigned)up << 23);
            const _Float16 hi = (_Float16)x;
            sm.p[g][slot] = hi;
            sm.p[kG + g][slot] = (_Float16)(x - (float)hi);
            if (lane == 0) {
                sm.ml[g][0] = m;
                sm.ml[g][1] = l;
                sm.pinv[g] = __uint_as_float((unsigned)(254 - up) << 23);
            }
        }
    }
    __syncthreads();

    // ---- O^T = V^T P^T: wave w owns dims 32 w .. 32 w + 31 (two 16-dim tiles, two 32-position steps)
    ts.mark(2);
    const bool direct = a.direct_out && nact == 1;  // operator API, one split: no merge needed
    Ws ws = ws_carve(a.workspace, a.heads, ns);
    const int h = h0 + hd;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int dt = 32 * wave + 16 * t;
        f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            h8 av;
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = sm.v[32 * st + c4 + 4 * i][dt + r16];
            const h8 bv = *reinterpret_cast<const h8*>(&sm.p[r16][32 * st + 8 * c4]);
            o = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, o, 0, 0, 0);
        }
        // lane (column r16, c4) holds dims dt + 4 c4 + r of its column
        const float inv = sm.pinv[hd];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = (o[r] + row_ror<8>(o[r])) * inv;
            if (lo || !live) continue;
            const int d = dt + 4 * c4 + r;
            if (direct) a.out[(size_t)h * D + d] = v / sm.ml[hd][1];
            else PlainIO::st(ws.o + ((size_t)h * ns + split) * D + d, v);
        }
    }
    if (direct) return;
    if (tid < group) {
        PlainIO::st(ws.ml + ((size_t)(h0 + tid) * ns + split) * 2 + 0, sm.ml[tid][0]);
        PlainIO::st(ws.ml + ((size_t)(h0 + tid) * ns + split) * 2 + 1, sm.ml[tid][1]);
    }
    // engine path: split 0 seeds the fixed-point residual accumulator of the o_proj with the
    // slices attn_body's workgroups of heads h0 .. h0 + group - 1 seed
    if (a.xacc != nullptr && split == 0) {
        const int per = (a.hidden + a.heads - 1) / a.heads;
        for (int i = h0 * per + tid; i < min((h0 + group) * per, a.hidden); i += kThreads)
            PlainIO::st_ll(a.xacc + i, a.resid_scale == 0.f ? 0ll
                                       : a.resid_fixed       ? a.resid_fixed[i]
                                                             : to_fixed(a.resid[i]));
    }
}

}  // namespace

bool attn_gqa_supported(const AttnArgs& a) {
    if (CH != kP || a.head_dim != D || a.kv_heads <= 0 || a.heads <= 0 || a.heads % a.kv_heads != 0) return false;
    const int group = a.heads / a.kv_heads;
    if (group < 2 || group > kG) return false;
    // an fp32 cache's values are not exact in fp16
    if (a.cache_dtype != LLMI_F16 && a.cache_dtype != LLMI_I8) return false;
    if (a.publish || a.qkv_tag != nullptr) return false;  // the fused q/k/v launch's forms
    return (uintptr_t)a.k_cache % 16 == 0 && (uintptr_t)a.v_cache % 16 == 0;  // 16-byte row chunks
}

int attn_gqa_launch(const AttnArgs& a, hipStream_t s) {
    LLMI_REQUIRE(attn_gqa_supported(a),
                 "attn_gqa: head_dim 128, 2 <= heads / kv_heads <= 8 and a 16-byte aligned f16 or i8 cache only");
    const int ns = (a.max_seq + CH - 1) / CH;  // (pointers, max_seq, nact and pos: attn_decode_launch checked them)
    const bool hs = a.nact > 0;
    const dim3 grid(a.kv_heads, hs ? a.nact : ns);
    if (a.cache_dtype == LLMI_I8) {
        LLMI_REQUIRE(a.k_scale && a.v_scale && (uintptr_t)a.k_scale % 2 == 0 && (uintptr_t)a.v_scale % 2 == 0,
                     "attn_gqa: an int8 cache needs its row scales (k_scale, v_scale)");
        if (hs) hipLaunchKernelGGL((attn_gqa_kernel<int8_t, true>), grid, dim3(kThreads), 0, s, a, ns);
        else hipLaunchKernelGGL((attn_gqa_kernel<int8_t, false>), grid, dim3(kThreads), 0, s, a, ns);
    } else {
        if (hs) hipLaunchKernelGGL((attn_gqa_kernel<__half, true>), grid, dim3(kThreads), 0, s, a, ns);
        else hipLaunchKernelGGL((attn_gqa_kernel<__half, false>), grid, dim3(kThreads), 0, s, a, ns);
    }
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace llmi
