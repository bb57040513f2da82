// Prefill linear layers, int8 weights (W8A16), on the matrix cores with LDS-DMA staging:
//   Y[m, n] (op)= s[n] * sum_p sum_k A_p[m, k] * q[n, k]      (nn.Linear, q row-major [out, in])
// the int8 engine's form of gemm2.hip's GEMM (launchLinearGemm, linear.cu:38-99, for a weight
// quantised on load: quant.hip / load_synthetic, one fp16 scale per output row).
//
// Numerics. int8 values are exact in fp16, so q enters v_mfma_f32_16x16x32_f16 exactly; the
// activations arrive as P fp16 planes (gemm2.hip: P = 2 is fp32-faithful, P = 1 the fp16
// throughput mode) and every product is accumulated in fp32. The row scale is applied once,
// in fp32, in the epilogue (as gemm.hip does) -- per K slice under EPI_SLAB, which is linear,
// and to the gate and the up column each with its own row's scale before the SiLU.
//
// Structure for gfx950. A BM x 128 output tile per 256-thread workgroup (BM 64 or 128; 4 waves,
// 2 x 2, each (BM/2) x 64), operands staged global -> LDS by global_load_lds_dwordx4 (no VGPRs,
// no ds_write pass), the LDS image lane-linear with gemm2's XOR swizzle on the global SOURCE
// address.
//  * Two rings at a 2 : 1 ratio. A 128-row x 128-byte int8 B tile is the image that swizzle
//    was built for and covers K = 128; an A stage (128-B rows of fp16) covers K = 64. So the
//    K loop runs in A steps of 64, and B stage s serves A steps 2 s and 2 s + 1 (its bytes
//    0..63 and 64..127). DMA group g = A stage g, plus B stage g / 2 when g is even. The A
//    ring has 3 slots and the B ring 2: group g + 2 is issued at step g, right after the
//    barrier that ends step g - 1 -- its A slot (g + 2) % 3 was last read in step g - 1, its
//    B slot (g / 2 + 1) & 1 in steps g - 2 and g - 1.
//  * vmcnt. The groups alternate in size: GE = P * BM / 32 + 4 DMA instructions per thread
//    for an even group, GO = P * BM / 32 for an odd one. Before the barrier of step g exactly
//    group g + 1 may stay in flight, so an even step waits for vmcnt(GO) and an odd one for
//    vmcnt(GE) -- or 0 when nothing follows. K / 64 is even (K a multiple of 128): the loop
//    is written two steps at a time and both counts are immediates.
//  * int8 -> fp16 in registers. A lane's ds_read_b128 of B holds 16 consecutive k of one
//    column. Each dword x of it becomes two packed-half dwords: v_perm_b32 of x ^ 0x80808080
//    against 0x64646464 builds the halves 0x6400 | (q + 128) = 1024 + 128 + q, and one packed
//    fp16 add of -1152 leaves q, exactly (all three values are integers below 2048). Five
//    VALU operations per four weights, no v_cvt. The column loop is outermost in a step and
//    the A fragments are held in registers, so the conversion of column fragment j + 1 has
//    no dependence on, and is scheduled among, the MFMAs of fragment j.
//  * Fragment k order. The 16 bytes of lane group fq (lane >> 4) are k = 16 fq .. 16 fq + 15
//    of the step: bytes 0..7 feed one MFMA, bytes 8..15 the next. The matching A fragments
//    are the 16-B chunks 2 fq and 2 fq + 1 of the A row (gemm2 reads chunks fq and 4 + fq):
//    within a step the contraction order over k is permuted, identically for A and B.
//  * Workgroup ids are remapped (bijectively) so consecutive tiles share an XCD; split-K
//    slices of a tile are consecutive ids. M is ragged: row loads clamp, stores are masked.
// No 256 x 256 ping-pong form (gemm3's) exists for int8 weights.
// Roofline: MFMA (fp16 dense 2.5 PFLOP/s); FLOPs per launch 2 * M * N * K (P = 2 issues 2x
// that on the matrix cores); weight bytes N * K, half of gemm2's.
#include <cstdint>

#include "kernels.h"

namespace llmi {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBN = 128;
constexpr int kBKA = 64;    // K of an A stage (128-B rows of fp16)
constexpr int kBKB = 128;   // K of a B stage (128-B rows of int8)
constexpr int kRowB = 128;  // LDS row bytes, both operands
constexpr int kAS = 3;      // A ring slots
constexpr int kBS = 2;      // B ring slots
constexpr int kBBytes = kBN * kRowB;
constexpr int kBGL = kBBytes / (kThreads * 16);  // B DMA instructions per thread per stage

// gemm2's LDS image swizzle: 16-B chunk c of 128-B row r is stored at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int swz(int b) { return b ^ (((b >> 8) & 7) << 4); }

// 16-B LDS-DMA as inline asm (M0 saved/restored): hipcc neither counts it nor waits for it
// (gemm2.hip)
__device__ __forceinline__ void glds16(const void* g, unsigned lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(lds)
                 : "memory");
}
__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

// gemm2's gate/up pairing: tile row tr holds gate column g0 + 32 (tr >> 6) + (tr & 31) for
// (tr & 32) == 0, its up row (+ pair_off) otherwise
__device__ __forceinline__ int b_src_row(int epi, int n0, int tr, int pair_off) {
    if (epi != EPI_SILU_MUL) return n0 + tr;
    const int gc = n0 + 32 * (tr >> 6) + (tr & 31);
    return (tr & 32) ? pair_off + gc : gc;
}

// 16 int8 (k ascending) -> two h8 fragments, exactly
__device__ __forceinline__ void cvt16(const u32x4 raw, h8& f0, h8& f1) {
    union { h8 v; uint32_t u[4]; } o[2];
    const h2 bias = {(_Float16)-1152.0f, (_Float16)-1152.0f};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t x = raw[d] ^ 0x80808080u;
        union { uint32_t u; h2 h; } lo, hi;
        lo.u = __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u);  // bytes 0, 1 under 0x64
        hi.u = __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u);  // bytes 2, 3
        lo.h += bias;
        hi.h += bias;
        o[d >> 1].u[2 * (d & 1)] = lo.u;
        o[d >> 1].u[2 * (d & 1) + 1] = hi.u;
    }
    f0 = o[0].v;
    f1 = o[1].v;
}

template <int BM, int P, int EPI>
__global__ __launch_bounds__(kThreads) void gemm_w8_kernel(GemmW8Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int A_BYTES = BM * kRowB;  // one plane of one A stage
    constexpr int A_STAGE = P * A_BYTES;
    constexpr int A_GL = A_BYTES / (kThreads * 16);  // DMA instructions per thread per plane
    constexpr int GO = P * A_GL;                     // an odd group: the A stage alone
    constexpr int GE = GO + kBGL;                    // an even group: A and B
    constexpr int B_BASE = kAS * A_STAGE;
    constexpr int MI = BM / 32;  // 16-row fragments per wave

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wc = w & 1;

    // bijective XCD remap: blocks sharing bid % 8 get consecutive tile ids
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int S = (EPI == EPI_SLAB) ? a.ksplit : 1;  // split-K: slices of one tile are consecutive ids
    const int tile = id / S, slice = id - tile * S;
    const int rt = tile / a.n_tiles, ct = tile - rt * a.n_tiles;
    const int m0 = rt * BM;
    const int n0 = (EPI == EPI_SILU_MUL) ? ct * (kBN / 2) : ct * kBN;
    const int K = a.k / S;  // this slice's K extent, from k_begin
    const int k_begin = slice * K;

    // per-thread DMA sources: instruction j of this thread fills LDS bytes j * 4096 + 16 t
    // (lane-linear); that slot holds logical byte swz(.) of the tile
    const char* a_src[P][A_GL];
    const char* b_src[kBGL];
#pragma unroll
    for (int j = 0; j < A_GL; ++j) {
        const int b = swz(j * kThreads * 16 + t * 16);
        const int row = min(m0 + (b >> 7), a.m - 1);
#pragma unroll
        for (int p = 0; p < P; ++p)
            a_src[p][j] = reinterpret_cast<const char*>(a.a[p]) + ((size_t)row * a.lda + k_begin) * 2 + (b & 127);
    }
#pragma unroll
    for (int j = 0; j < kBGL; ++j) {
        const int b = swz(j * kThreads * 16 + t * 16);
        const int src = b_src_row(EPI, n0, b >> 7, a.pair_off);
        b_src[j] = reinterpret_cast<const char*>(a.w) + (size_t)src * a.k + k_begin + (b & 127);
    }
    const unsigned lds_base = (unsigned)(uintptr_t)lds + w * 1024;
    // group g: A stage g into A slot sa; with_b: B stage g / 2 into B slot sb
    auto issue = [&](int g, int sa, int sb, bool with_b) {
        const unsigned ab = __builtin_amdgcn_readfirstlane(lds_base + sa * A_STAGE);  // wave-uniform
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < A_GL; ++j)
                glds16(a_src[p][j] + (size_t)g * (kBKA * 2), ab + p * A_BYTES + j * kThreads * 16);
        if (with_b) {
            const unsigned bb = __builtin_amdgcn_readfirstlane(lds_base + B_BASE + sb * kBBytes);
#pragma unroll
            for (int j = 0; j < kBGL; ++j) glds16(b_src[j] + (size_t)(g >> 1) * kBKB, bb + j * kThreads * 16);
        }
    };

    f4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    // one A step: half h (0 / 1) of B slot sb against A slot sa
    auto step = [&](int sa, int sb, int h) {
        const char* As = lds + sa * A_STAGE;
        const char* Bs = lds + B_BASE + sb * kBBytes;
        u32x4 raw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            raw[j] = *reinterpret_cast<const u32x4*>(Bs + swz((wc * 64 + j * 16 + fr) * kRowB + (4 * h + fq) * 16));
        h8 af[MI][P][2];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ab = swz((wr * (BM / 2) + i * 16 + fr) * kRowB + (2 * fq + u) * 16);
#pragma unroll
                for (int p = 0; p < P; ++p) af[i][p][u] = *reinterpret_cast<const h8*>(As + p * A_BYTES + ab);
            }
        h8 bf[2][2];
        cvt16(raw[0], bf[0][0], bf[0][1]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < 3) cvt16(raw[j + 1], bf[(j + 1) & 1][0], bf[(j + 1) & 1][1]);  // among fragment j's MFMAs
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][p][u], bf[j & 1][u], acc[i][j], 0, 0, 0);
        }
    };

    const int KT = K / kBKA;  // even, >= 2
    issue(0, 0, 0, true);
    issue(1, 1, 0, false);
    int sa = 0;  // A slot of the even step
    for (int kt = 0; kt < KT; kt += 2) {
        const int sb = (kt >> 1) & 1;
        const int sa1 = sa == kAS - 1 ? 0 : sa + 1, sa2 = sa1 == kAS - 1 ? 0 : sa1 + 1;
        // even step: group kt landed in every wave (group kt + 1, GO instructions, stays in
        // flight), then the raw barrier publishes it; every wave has also finished step kt - 1
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(GO) : "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < KT) issue(kt + 2, sa2, sb ^ 1, true);
        step(sa, sb, 0);
        // odd step: group kt + 1 landed (group kt + 2, GE instructions, in flight if issued)
        if (kt + 2 < KT) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(GE) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (kt + 3 < KT) issue(kt + 3, sa, sb ^ 1, false);  // A slot (kt + 3) % 3 == kt % 3, read last in the even step
        step(sa1, sb, 1);
        sa = sa2;
    }

    // epilogue: C fragment (i, j) register r is row 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15)
    if (EPI == EPI_SILU_MUL) {
        float sg[2], su[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gc = n0 + 32 * wc + 16 * j + fr;
            sg[j] = __half2float(a.scales[gc]);
            su[j] = __half2float(a.scales[a.pair_off + gc]);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int m = m0 + wr * (BM / 2) + 16 * i + 4 * fq + r4;
                if (m >= a.m) continue;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int gc = n0 + 32 * wc + 16 * j + fr;
                    const float v = silu_f(acc[i][j][r4] * sg[j]) * (acc[i][j + 2][r4] * su[j]);
                    const size_t o = (size_t)m * a.ldy + gc;
                    if (a.y_hi) {  // the down GEMM's input planes, written directly
                        const _Float16 hi = (_Float16)v;
                        a.y_hi[o] = hi;
                        if (a.y_lo) a.y_lo[o] = (_Float16)(v - (float)hi);
                    } else {
                        a.y[o] = v;
                    }
                }
            }
    } else {
        float sc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = __half2float(a.scales[n0 + wc * 64 + 16 * j + fr]);
        float* ybase = EPI == EPI_SLAB ? a.slab + (size_t)slice * a.m * a.ldy : a.y;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int m = m0 + wr * (BM / 2) + 16 * i + 4 * fq + r4;
                if (m >= a.m) continue;
                float* yrow = ybase + (size_t)m * a.ldy;
#pragma unroll
                for (int j = 0; j < 4; ++j) yrow[n0 + wc * 64 + 16 * j + fr] = acc[i][j][r4] * sc[j];
            }
    }
}

template <int BM, int P, int EPI>
int launch3(const GemmW8Args& a, int grid, hipStream_t s) {
    constexpr size_t lds = (size_t)kAS * P * BM * kRowB + (size_t)kBS * kBBytes;
    static const bool attr = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w8_kernel<BM, P, EPI>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
    }();
    LLMI_REQUIRE(attr, "gemm_w8: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL((gemm_w8_kernel<BM, P, EPI>), dim3(grid), dim3(kThreads), lds, s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

template <int BM, int P>
int launch2(const GemmW8Args& a, int grid, hipStream_t s) {
    switch (a.epi) {
        case EPI_STORE: return launch3<BM, P, EPI_STORE>(a, grid, s);
        case EPI_SILU_MUL: return launch3<BM, P, EPI_SILU_MUL>(a, grid, s);
        default: return launch3<BM, P, EPI_SLAB>(a, grid, s);
    }
}

}  // namespace

bool gemm_w8_supported(int n, int k, int epi, int ksplit) {
    if (epi != EPI_STORE && epi != EPI_SLAB && epi != EPI_SILU_MUL) return false;
    const int ncols = (epi == EPI_SILU_MUL) ? n / 2 : n;
    const int tile = (epi == EPI_SILU_MUL) ? kBN / 2 : kBN;
    const int ks = epi == EPI_SLAB ? ksplit : 1;
    return n > 0 && k > 0 && ks >= 1 && ncols % tile == 0 && (epi != EPI_SILU_MUL || n % 2 == 0) &&
           k % (ks * kBKB) == 0;
}

int gemm_w8_launch(GemmW8Args a, hipStream_t s) {
    LLMI_REQUIRE(a.a[0] && a.w && a.m > 0, "gemm_w8: null operand or empty M");
    LLMI_REQUIRE(a.scales != nullptr, "gemm_w8: int8 weights need per-row scales");
    LLMI_REQUIRE(a.planes == 1 || (a.planes == 2 && a.a[1]), "gemm_w8: planes must be 1 or 2 (with a[1])");
    if (!gemm_w8_supported(a.n, a.k, a.epi, a.ksplit)) {
        set_last_error("[llmi][ERROR] gemm_w8: store, slab or silu_mul; N a multiple of 128 (gate_up: 2 x 64), "
                       "K / ksplit a multiple of 128");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_REQUIRE(a.epi == EPI_SILU_MUL ? (a.y || a.y_hi) : a.epi == EPI_SLAB ? a.slab != nullptr : a.y != nullptr,
                 "gemm_w8: null output");
    LLMI_REQUIRE(a.lda >= a.k && a.lda % 8 == 0 && (reinterpret_cast<uintptr_t>(a.a[0]) & 15) == 0 &&
                     (a.planes == 1 || (reinterpret_cast<uintptr_t>(a.a[1]) & 15) == 0),
                 "gemm_w8: A planes must be 16-B aligned with lda >= k, lda % 8 == 0");
    LLMI_REQUIRE((reinterpret_cast<uintptr_t>(a.w) & 15) == 0, "gemm_w8: W must be 16-B aligned");
    LLMI_REQUIRE(a.epi != EPI_SILU_MUL || a.pair_off == a.n / 2, "gemm_w8: gate_up pair offset must be N / 2");
    const int ncols = (a.epi == EPI_SILU_MUL) ? a.n / 2 : a.n;
    LLMI_REQUIRE(a.ldy >= ncols, "gemm_w8: ldy must cover the output columns");
    a.n_tiles = ncols / ((a.epi == EPI_SILU_MUL) ? kBN / 2 : kBN);
    if (a.epi != EPI_SLAB) a.ksplit = 1;
    // 128-row tiles unless that leaves CUs idle (gemm2's rule; split-K supplies the workgroups)
    const int bm = a.epi == EPI_SLAB || ((a.m + 127) / 128) * a.n_tiles >= 256 ? 128 : 64;
    const int grid = ((a.m + bm - 1) / bm) * a.n_tiles * a.ksplit;
    if (bm == 128) return a.planes == 2 ? launch2<128, 2>(a, grid, s) : launch2<128, 1>(a, grid, s);
    return a.planes == 2 ? launch2<64, 2>(a, grid, s) : launch2<64, 1>(a, grid, s);
}

}  // namespace llmi
