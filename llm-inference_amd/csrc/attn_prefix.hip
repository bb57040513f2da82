// Shared-prefix decode attention for forked batch slots (opt-in: Batch option "prefix_attn";
// llmi_debug_attn_oproj_batch with prefix_group set; DESIGN.md §3 "Shared-prefix attention").
// Batch::fork gives n slots the same leading cache rows, copied physically, and attn_batch.hip
// then reads those identical rows n times a step. Here the members of a fork group read the
// group's first P rows (a multiple of 64: whole splits) ONCE, from the cache of the group's
// lowest-numbered member, the leader. Which member leads never matters: the rows are bitwise equal.
//
// One launch, a 1-d grid, prefix workgroups first:
//   prefix workgroup = (served group, kv head, split below P / 64): loads the split's 64 K rows and
// 64 V rows of the leader (fp16, or int8 with its row scales) and serves every query row, i.e.
// every (member, query head of this kv head) pair, rho = member * g + head, m * g <= 64 of them.
// Every member's position is >= P, so the split is full, holds no stale row and never the current
// one: no cache write, no xacc seed, no error word here.
//   tail workgroup = (slot, query head, split from skip[slot] on): attn_body's host-sized form on
// the slot's own arguments, as attn_batch_kernel calls it, skip = P / 64 for a member and 0 for a
// slot of no served group. It writes the cache row, and the first tail split seeds xacc and
// reports a split-count mismatch (attn_body's `first`).
// Each (member, head, split) partial O[128], m, l lands in that member's own workspace (ws_carve),
// so oproj_batch_launch merges behind it unchanged. No inter-workgroup waits: a plain grid.
//
// The prefix arithmetic is attn_gqa.hip's with query rows in the MFMA columns where it has the
// heads of one kv head. K: lane (r = lane % 16, c = lane / 16) of wave w loads the 16-byte chunks
// 4 s + c of row 16 w + r; the chunks ARE its A operands of v_mfma_f32_16x16x32_f16 (int8:
// converted once, exactly) and stay in registers for every pass. V goes once into the padded
// row-major fp16 image in LDS ([64][128 + 16], attn_gqa.hip's bank map) and stays for every pass.
// A pass is 8 query rows: column h is hi = fp16(q), column 8 + h is lo = fp16(q - hi) of the row's q,
// rotated at ITS member's device position into LDS as fp32 (waves take rows w, w + 4); scores
// = the fp32 tile's column h + column 8 + h, * s_k[j] for int8 (the scale stays outside the
// product), / sqrt(d); the fp32 softmax per row by one wave; p (int8: p s_v) scaled by the power of
// two that puts the row's largest weight in [2^13, 2^14) and split into two fp16 planes; O^T = V^T P^T
// with wave w on dims 32 w .. 32 w + 31. The next pass's q, position and rotation are fetched into
// registers while this pass computes. All K/V loads are issued before any position is read.
// HBM is read once; 3 barriers a pass.
//
// LDS 27,232 B dynamic (q 4 KiB, scores 2 KiB, V image 18 KiB, p planes 2.25 KiB, (m, l), the rows'
// targets); the tail's 10,000 B overlay it. hipcc remarks (gfx950), one kernel holding both bodies:
// 92 VGPRs (fp16 cache) / 98 (int8), no scratch, no spills, occupancy 5 / 4 waves a SIMD (fp16: the
// LDS bound of five workgroups a CU; int8: the VGPR bound).
#include "attn_impl.h"

namespace llmi {
namespace {

using namespace attn_detail;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kP = 64;       // positions of a workgroup: the split of the workspace (CH)
constexpr int kR = 8;        // query rows of a pass (two planes: 16 MFMA columns)
constexpr int kVS = D + 16;  // halves of a V image row: 72 words (attn_gqa.hip)
constexpr int kPS = kP + 8;  // halves of a p plane row

struct PfxLds {
    float q[kR][D];   // rotated q of the pass's rows (fp32, unscaled)
    float s[kR][kP];  // scores
    alignas(16) _Float16 v[kP][kVS];
    alignas(16) _Float16 p[2 * kR][kPS];  // [plane * 8 + row][k slot]
    float ml[kR][2];
    float pinv[kR];       // 2^-e of the row's planes
    float* o[2][kR];      // by pass parity: the row's O[128] in its member's workspace
    float* mlp[2][kR];    // ... and its (m, l)
};
constexpr size_t kPrefixLds = sizeof(PfxLds) > kAttnLds ? sizeof(PfxLds) : kAttnLds;

// 8 int8 -> 8 fp16, exact (attn_gqa.hip, gemv_rows_mfma.hip): byte b ^ 0x80 under the exponent byte of fp16 1024
__device__ __forceinline__ h8 i8x8_to_h8(uint32_t w0, uint32_t w1) {
    const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
    const uint32_t x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
    const h2 r0 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04010400u)) - bias;
    const h2 r1 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04030402u)) - bias;
    const h2 r2 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04010400u)) - bias;
    const h2 r3 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04030402u)) - bias;
    return (h8){r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
}

// a wave's two query rows of a pass as fetched: the raw pair (i, i + d/2) and its rotation
struct QFetch {
    float q0[2], q1[2], c[2], s[2];
};

// prefix workgroup (served group gi, kv head, split); ns: the workspace's split stride
template <typename KT>
__device__ __forceinline__ void prefix_body(const AttnBatchArgs& b, const AttnPrefixPlan& pl, int gi, int kvh,
                                            int split, int ns, PfxLds& sm) {
    constexpr bool Q8 = kQ8<KT>;
    constexpr int NK = Q8 ? 2 : 4;   // 16-byte chunks of a row per lane
    constexpr int CD = Q8 ? 16 : 8;  // dims of a chunk
    const AttnArgs& a = b.a;
    const AttnPrefixPlan::Group& G = pl.g[gi];
    const int group = a.heads / a.kv_heads, h0 = kvh * group;
    const int R = G.n * group;  // query rows: (member, head of the kv head)
    const int npass = (R + kR - 1) / kR;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, c4 = lane >> 4;
    const int start = split * kP;
    const int jrow = start + 16 * wave + r16;  // the cached row whose chunks this lane loads (< P <= max_seq)
    const AttnBatchSlot& lead = b.slot[G.member[0]];
    const KT* kc = reinterpret_cast<const KT*>(lead.k_cache) + (size_t)kvh * a.max_seq * D;
    const KT* vc = reinterpret_cast<const KT*>(lead.v_cache) + (size_t)kvh * a.max_seq * D;

    // ---- every K and V load of the split, before any member's position is read
    uint4 kr[NK], vr[NK];
    __half ksr[4], vsr = __ushort_as_half(0);  // int8: scales of the C tile's rows / of row `lane`
    (void)ksr;
    {
        const KT* kp = kc + (size_t)jrow * D + c4 * CD;
        const KT* vp = vc + (size_t)jrow * D + c4 * CD;
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            kr[s] = ld_nt16(kp + 4 * s * CD);
            vr[s] = ld_nt16(vp + 4 * s * CD);
        }
        if constexpr (Q8) {
            const __half* ksc = lead.k_scale + (size_t)kvh * a.max_seq;
            const __half* vsc = lead.v_scale + (size_t)kvh * a.max_seq;
#pragma unroll
            for (int r = 0; r < 4; ++r) ksr[r] = ksc[start + 16 * wave + 4 * c4 + r];
            vsr = vsc[start + lane];
        }
    }

    // ---- q of rows wave, wave + 4 of a pass: the member's position (clamped to the table: the
    // host validates it, the tail reports a mismatch), the raw pair, cos and sin. Wave-uniform row.
    auto row_slot = [&](int rho) -> const AttnBatchSlot& { return b.slot[G.member[rho / group]]; };
    auto fetch = [&](int pass, QFetch& f) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rho = kR * pass + wave + 4 * u;
            f.q0[u] = f.q1[u] = f.s[u] = 0.f;
            f.c[u] = 1.f;
            if (rho >= R) continue;
            const AttnBatchSlot& sl = row_slot(rho);
            int z = 0;
            asm volatile("" : "+v"(z));  // a per-lane load: the position stays in a VGPR (attn_body)
            const int pos = min(max(sl.pos_dev[z], 0), a.max_seq - 1);
            const float* qrow = sl.qkv + (size_t)(h0 + rho % group) * D;
            f.q0[u] = qrow[lane];
            f.q1[u] = qrow[lane + D / 2];
            if (a.rope_tab) {
                const float2 cs = reinterpret_cast<const float2*>(a.rope_tab)[(size_t)pos * (D / 2) + lane];
                f.c[u] = cs.x;
                f.s[u] = cs.y;
            } else if (a.rope) {
                rope_cs(pos, lane, D, a.rope_base, &f.c[u], &f.s[u]);
            }
        }
    };
    auto put = [&](int pass, const QFetch& f) {  // attn_body's rotation; the row's targets
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int rr = wave + 4 * u, rho = kR * pass + rr;
            if (rho >= R) continue;
            sm.q[rr][lane] = f.q0[u] * f.c[u] - f.q1[u] * f.s[u];
            sm.q[rr][lane + D / 2] = f.q1[u] * f.c[u] + f.q0[u] * f.s[u];
            if (lane == 0) {
                Ws ws = ws_carve(row_slot(rho).workspace, a.heads, ns);
                const size_t at = (size_t)(h0 + rho % group) * ns + split;
                sm.o[pass & 1][rr] = ws.o + at * D;
                sm.mlp[pass & 1][rr] = ws.ml + at * 2;
            }
        }
    };
    QFetch qf;
    fetch(0, qf);

    // ---- the K operands (registers, every pass) and the V image (LDS, every pass)
    h8 kop[4];
    {
        _Float16* vimg = &sm.v[16 * wave + r16][0];
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const int d0 = (4 * s + c4) * CD;
            if constexpr (Q8) {
                kop[2 * s] = i8x8_to_h8(kr[s].x, kr[s].y);
                kop[2 * s + 1] = i8x8_to_h8(kr[s].z, kr[s].w);
                *reinterpret_cast<h8*>(vimg + d0) = i8x8_to_h8(vr[s].x, vr[s].y);
                *reinterpret_cast<h8*>(vimg + d0 + 8) = i8x8_to_h8(vr[s].z, vr[s].w);
            } else {
                kop[s] = __builtin_bit_cast(h8, kr[s]);
                *reinterpret_cast<h8*>(vimg + d0) = __builtin_bit_cast(h8, vr[s]);
            }
        }
    }

    const int hd = r16 & 7;  // this lane's B / C column: row hd of the pass, plane lo
    const bool lo = r16 >= 8;
    const float qscale = 1.0f / sqrtf((float)D);
    // position lane = 32 st + c + 4 i sits in k slot 32 st + 8 c + i (attn_gqa.hip)
    const int slot = (lane & 32) + 8 * (lane & 3) + ((lane & 31) >> 2);

    for (int pass = 0; pass < npass; ++pass) {
        put(pass, qf);
        if (pass + 1 < npass) fetch(pass + 1, qf);  // in flight across this pass
        __syncthreads();  // (pass 0: the V image too)

        // ---- scores of positions 16 w .. 16 w + 15 for the pass's rows
        const bool live = kR * pass + hd < R;
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int d0 = Q8 ? (4 * (o / 2) + c4) * CD + 8 * (o % 2) : (4 * o + c4) * CD;
            h8 bq;  // the planes' 8 dims from d0 of column r16
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = live ? sm.q[hd][d0 + i] : 0.f;
                const _Float16 hi = (_Float16)v;
                bq[i] = lo ? (_Float16)(v - (float)hi) : hi;
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kop[o], bq, acc, 0, 0, 0);
        }
        // lane (column r16, c4) holds positions 16 w + 4 c4 + r of its column: lo + hi, the scales
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sc = acc[r] + row_ror<8>(acc[r]);
            if constexpr (Q8) sc *= __half2float(ksr[r]);  // the row's scale after the integer sum
            sc *= qscale;
            if (!lo && live) sm.s[hd][16 * wave + 4 * c4 + r] = sc;
        }
        __syncthreads();

        // ---- fp32 softmax over the split's 64 positions, a wave per row, and the planes of p
        for (int rr = wave; rr < kR; rr += kThreads / kWave) {
            if (kR * pass + rr >= R) {  // unused columns are zero
                sm.p[rr][lane] = (_Float16)0.f;
                sm.p[kR + rr][lane] = (_Float16)0.f;
                continue;
            }
            const float s = sm.s[rr][lane];
            const float m = wave_max(s);
            const float p = expf(s - m);
            const float l = wave_sum(p);
            float pw = p;
            if constexpr (Q8) pw = p * __half2float(vsr);  // s_v folded into p
            // 2^e with max(pw) * 2^e in [2^13, 2^14): biased exponents, exact both ways
            const int ex = (int)((__float_as_uint(wave_max(pw)) >> 23) & 0xffu);
            const int up = min(max(267 - ex, 1), 253);
            const float x = pw * __uint_as_float((unsigned)up << 23);
            const _Float16 hi = (_Float16)x;
            sm.p[rr][slot] = hi;
            sm.p[kR + rr][slot] = (_Float16)(x - (float)hi);
            if (lane == 0) {
                sm.ml[rr][0] = m;
                sm.ml[rr][1] = l;
                sm.pinv[rr] = __uint_as_float((unsigned)(254 - up) << 23);
            }
        }
        __syncthreads();

        // ---- O^T = V^T P^T: wave w owns dims 32 w .. 32 w + 31 (two 16-dim tiles, two 32-position steps)
        float* orow = sm.o[pass & 1][hd];
        const float inv = sm.pinv[hd];
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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (o[r] + row_ror<8>(o[r])) * inv;
                if (!lo && live) PlainIO::st(orow + dt + 4 * c4 + r, v);
            }
        }
        if (tid < kR && kR * pass + tid < R) {
            PlainIO::st(sm.mlp[pass & 1][tid] + 0, sm.ml[tid][0]);
            PlainIO::st(sm.mlp[pass & 1][tid] + 1, sm.ml[tid][1]);
        }
        // (no barrier: what the next pass writes before its first barrier -- q, the other parity's
        // targets -- was last read before this pass's second; ml / pinv / p are written behind its
        // second and third, which every wave reaches only after this point)
    }
}

template <typename KT>
__global__ __launch_bounds__(kThreads) void attn_prefix_kernel(AttnBatchArgs b, AttnPrefixPlan pl, int ns) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int bid = blockIdx.x;
    if (bid < pl.n_pfx) {
        int gi = 0;
        for (int i = 1; i < pl.n_groups; ++i)
            if (bid >= pl.g[i].wg0) gi = i;
        const int local = bid - pl.g[gi].wg0;
        prefix_body<KT>(b, pl, gi, local % b.a.kv_heads, local / b.a.kv_heads, ns, *reinterpret_cast<PfxLds*>(smem));
        return;
    }
    // tail: attn_batch_kernel's workgroup (slot, head, split) with the splits counted from skip
    const int t = bid - pl.n_pfx;
    const int h = t % b.a.heads, y = (t / b.a.heads) % pl.top, si = t / (b.a.heads * pl.top);
    const AttnBatchSlot& sl = b.slot[si];
    const int first = pl.skip[si], split = first + y;
    if (split >= sl.nact) return;  // this slot's context ends before the split
    AttnArgs a = b.a;
    a.qkv = sl.qkv;
    a.k_cache = sl.k_cache; a.v_cache = sl.v_cache;
    a.k_scale = sl.k_scale; a.v_scale = sl.v_scale;
    a.pos_dev = sl.pos_dev; a.nact = sl.nact;
    a.workspace = sl.workspace;
    a.xacc = sl.xacc; a.resid = sl.resid; a.resid_fixed = sl.resid_fixed; a.resid_scale = sl.resid_scale;
    a.err = sl.err;
    attn_body<KT, PlainIO, true>(a, h, split, ns, smem, nullptr, first);
}

}  // namespace

AttnPrefixPlan attn_prefix_plan(const AttnPrefixArgs& p) {
    AttnPrefixPlan pl;
    const AttnArgs& a = p.b.a;
    const int n = p.b.n;
    for (int i = 0; i < kAttnBatchMax; ++i) pl.leader[i] = i;
    for (int i = 0; i < n && i < kAttnBatchMax; ++i) pl.top = std::max(pl.top, p.b.slot[i].nact);
    if (n < 2 || n > kAttnBatchMax || CH != kP || a.head_dim != D || a.heads <= 0 || a.kv_heads <= 0 ||
        a.heads % a.kv_heads != 0 || a.heads / a.kv_heads > kR || a.max_seq <= 0)
        return pl;
    if (a.cache_dtype != LLMI_F16 && a.cache_dtype != LLMI_I8) return pl;  // an fp32 cache's values are not exact in fp16
    if (a.direct_out || a.qkv_tag != nullptr || a.publish) return pl;
    for (int i = 0; i < n; ++i) {
        if (p.group[i] == 0 || pl.skip[i] != 0 || pl.n_groups == kAttnPrefixGroups) continue;
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || p.group[j] == p.group[i];
        if (seen) continue;  // (its group was refused at its first member)
        AttnPrefixPlan::Group g;
        int splits = a.max_seq / kP;
        bool ok = true;
        for (int j = i; j < n; ++j) {
            if (p.group[j] != p.group[i]) continue;
            const AttnBatchSlot& r = p.b.slot[j];
            ok = ok && r.nact > 0;
            splits = std::min(splits, std::min(p.rows[j] / kP, r.nact - 1));
            g.member[g.n++] = j;
        }
        const AttnBatchSlot& lead = p.b.slot[i];
        ok = ok && lead.k_cache && lead.v_cache && (uintptr_t)lead.k_cache % 16 == 0 && (uintptr_t)lead.v_cache % 16 == 0;
        if (a.cache_dtype == LLMI_I8)
            ok = ok && lead.k_scale && lead.v_scale && (uintptr_t)lead.k_scale % 2 == 0 && (uintptr_t)lead.v_scale % 2 == 0;
        if (!ok || g.n < 2 || splits < 1) continue;
        g.splits = splits;
        g.wg0 = pl.n_pfx;
        pl.n_pfx += a.kv_heads * splits;
        for (int k = 0; k < g.n; ++k) {
            pl.skip[g.member[k]] = splits;
            pl.leader[g.member[k]] = i;
        }
        pl.g[pl.n_groups++] = g;
    }
    pl.top = 0;
    for (int i = 0; i < n; ++i) pl.top = std::max(pl.top, p.b.slot[i].nact - pl.skip[i]);
    return pl;
}

bool attn_prefix_supported(const AttnPrefixArgs& p) { return attn_prefix_plan(p).n_groups > 0; }

int attn_prefix_launch(const AttnPrefixArgs& p, hipStream_t s) {
    const AttnPrefixPlan pl = attn_prefix_plan(p);
    if (pl.n_groups == 0) return attn_batch_launch(p.b, s);  // no group to serve: the batched launch itself
    const AttnArgs& a = p.b.a;
    // (the plan holds: n 2..8, head_dim 128, head counts, an f16 / i8 cache, direct_out 0, no granule rows)
    LLMI_REQUIRE(a.stamps == nullptr, "attn_prefix: no workgroup stamps");
    LLMI_REQUIRE((a.max_seq + CH - 1) / CH <= kMaxSplits, "attn_prefix: max_seq out of range");
    const int ns = (a.max_seq + CH - 1) / CH;
    for (int i = 0; i < p.b.n; ++i) {  // attn_batch_launch's checks of a slot
        const AttnBatchSlot& r = p.b.slot[i];
        LLMI_REQUIRE(r.qkv && r.k_cache && r.v_cache && r.workspace, "attn_prefix: a slot's qkv, cache or workspace is null");
        LLMI_REQUIRE(r.pos_dev && r.nact > 0 && r.nact <= ns,
                     "attn_prefix: every slot needs its device position and its host-sized nact (1..max_seq / 64)");
        LLMI_REQUIRE(!r.xacc || r.resid || r.resid_fixed, "attn_prefix: xacc seeding needs resid");
        if (a.cache_dtype == LLMI_I8) {
            LLMI_REQUIRE(r.k_scale && r.v_scale, "attn_prefix: an int8 cache needs its row scales (k_scale, v_scale)");
            LLMI_REQUIRE((uintptr_t)r.k_cache % 8 == 0 && (uintptr_t)r.v_cache % 8 == 0 &&
                             (uintptr_t)r.k_scale % 2 == 0 && (uintptr_t)r.v_scale % 2 == 0,
                         "attn_prefix: an int8 cache must be 8-byte aligned, its scales 2-byte");
        }
    }
    const dim3 grid(pl.n_pfx + a.heads * pl.top * p.b.n);  // (top >= 1: a member's last split is a tail)
    if (a.cache_dtype == LLMI_I8)
        hipLaunchKernelGGL((attn_prefix_kernel<int8_t>), grid, dim3(kThreads), kPrefixLds, s, p.b, pl, ns);
    else
        hipLaunchKernelGGL((attn_prefix_kernel<__half>), grid, dim3(kThreads), kPrefixLds, s, p.b, pl, ns);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace llmi
