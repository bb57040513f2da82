// Prefill linear layers, 4-bit group-quantised weights (W4A16, LLMI_I4), on the matrix cores with
// LDS-DMA staging:
//   Y[m, n] (op)= sum_g fp32(s[n, g]) * ( sum_{k in group g} sum_p A_p[m, k] * q[n, k] )
// the int4 engine's form of gemm_w8.hip's GEMM. The weight format is the decode GEMVs', read in
// place (llmi_quantize_groups_i4, include/llmi.h): groups of 128 columns, nibble q + 8 with the
// even column in the low nibble, rows of k / 2 bytes, fp16 scales in a separate [n][k / 128] array.
//
// Numerics. A nibble becomes the exact fp16 integer q in [-8, 7] (nibble 0 is -8) and enters
// v_mfma_f32_16x16x32_f16 as such; the activations arrive as P fp16 planes (P = 2 fp32-faithful,
// P = 1 the fp16 throughput mode); every product is accumulated in fp32. A group's partial sum
// is built in a group accumulator that the group's first MFMA starts from zero, and enters the
// main accumulator as acc += fp32(s) * gacc, once per group, in fp32 -- the order of the decode
// GEMV's chunks. q * s is never formed in fp16 (it has up to 15 significant bits). The epilogues
// apply no scale: under EPI_SLAB slice i holds the scaled sum of its own groups, and the gate and
// the up column are each fully scaled before the SiLU.
//
// Structure for gfx950: gemm_w8.hip's. A BM x 128 output tile per 256-thread workgroup (BM 64 or
// 128; 4 waves, 2 x 2, each (BM/2) x 64), operands staged global -> LDS by global_load_lds_dwordx4,
// the LDS image lane-linear with the swizzle on the global SOURCE address; one workgroup per CU.
//  * Two rings at a 2 : 1 ratio. An A stage is 128-B rows of fp16, K = 64, gemm2's XOR swizzle,
//    3 slots. A B stage is ONE scale group of the tile: 128 rows x 64 B = 8 KB, K = 128, 2 slots;
//    B stage s serves A steps 2 s and 2 s + 1 (its row bytes 0..31 and 32..63). K / 64 is even for
//    any K / ksplit that is a multiple of 128 -- an odd group count (the 7B down GEMM in two
//    slices: 43) needs nothing special, which a 128-B-row B stage (two groups) would.
//  * vmcnt. DMA group g = A stage g (GO = P * BM / 32 instructions per thread), plus B stage
//    g / 2 when g is even (2 more: 8 KB / (256 threads x 16 B); GE = GO + 2). Group g + 2 is
//    issued at step g, after the barrier that ends step g - 1 (its A slot (g + 2) % 3 was last
//    read in step g - 1, its B slot (g / 2 + 1) & 1 in steps g - 2 and g - 1). Loads return in
//    order, so before the barrier of step g the groups in flight are g (must land) and g + 1
//    (may stay): an even step waits for vmcnt(GO), the odd group g + 1; an odd step for
//    vmcnt(GE), the even group g + 1 -- or 0 when nothing follows. Both are immediates because
//    the loop is written two steps (one scale group) at a time.
//  * B swizzle. 64-B rows put two tile rows on a 128-B line and four on the 256 B that the 64
//    banks span, so gemm2's XOR does not apply. 16-B chunk c (0..3) of row r is stored at chunk
//    c ^ ((r >> 2) & 3) of its row. A fragment read is a ds_read_b64: lane (fr, fq) of column
//    fragment j takes bytes 32 h + 8 fq .. + 7 of row 16 j' + fr in A step h. The LDS serves a
//    b64 read 32 lanes at a time (fq 0, 1 or fq 2, 3): those read ONE logical chunk
//    c = 2 h + (fq >> 1), both 8-B halves, of 16 consecutive rows. Its 256-B bank position is
//    64 (r & 3) + 16 (c ^ ((r >> 2) & 3)) + 8 (fq & 1); over 16 rows (r & 3, (r >> 2) & 3) takes
//    all 16 values, so the 32 lanes cover 32 distinct 8-B slots: all 64 banks once, no conflict.
//  * Nibbles -> fp16 in registers, no v_cvt. A lane's 8 bytes are 16 consecutive k of one
//    column: bytes 0..3 feed one MFMA, bytes 4..7 the next, against the A row's 16-B chunks
//    2 fq and 2 fq + 1 (gemm_w8's k permutation inside a step, identical for A and B). A half
//    pair (k, k + 1) is one byte b: v_perm_b32 copies b to bytes 0 and 2, v_and_or_b32 with
//    0x00F0000F, 0x54006400 leaves 0x6400 | lo nibble = 1024 + n (the GEMV's trick) in the low
//    half and 0x5400 | hi nibble << 4 = 64 + n in the high half (fp16 64 has ulp 1/16, so the
//    nibble needs no shift), and one packed add of (-1032, -72) leaves (q_k, q_k+1) exactly.
//    3 VALU per 2 weights. The column loop is outermost in a step and the A fragments stay in
//    registers, so fragment j + 1 is converted among the MFMAs of fragment j.
//  * Scales. The tile's [groups][128] fp16 block (<= 14 KB for a 13B down slice) is staged in LDS
//    once, behind the first two DMA groups; a lane reads its four column scales per group with
//    ds_read_u16. This bounds K / ksplit by what LDS holds beside the rings: 192 groups (24576).
//    Loading a group ahead from global would mix compiler-counted loads into the hand-counted
//    vmcnt stream above.
//  * ISA counts (hipcc --save-temps; one K-loop iteration = one scale group = two A steps). The
//    P = 1, BM = 64 store instance: 32 MFMAs against 275 VALU instructions -- 64 v_perm_b32, 64
//    v_and_or_b32 and 64 v_pk_add_f16 of conversion, 32 v_accvgpr_read_b32 and 16 v_pk_fma_f32 of
//    group scaling, 4 v_cvt_f32_f16 of scales, the rest addresses: 8.6 VALU per MFMA, VALU-bound.
//    BM = 128: 343 VALU for 64 MFMAs (P = 1), 354 for 128 (P = 2). Registers (VGPRs + AGPRs,
//    scratch 0 in all twelve instances): 102 + 32, 124 + 32 (BM 64, P 1 / 2), 166 + 64, 204 + 64.
//  * Workgroup ids are remapped (bijectively) so consecutive tiles share an XCD; split-K
//    slices of a tile are consecutive ids. M is ragged: row loads clamp, stores are masked.
// Roofline: MFMA (fp16 dense 2.5 PFLOP/s); FLOPs per launch 2 * M * N * K (P = 2 issues 2x
// that); weight bytes N * K / 2 + N * K / 64 of scales.
#include <cstdint>

#include "kernels.h"

namespace llmi {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kBN = 128;
constexpr int kBKA = 64;    // K of an A stage (128-B rows of fp16)
constexpr int kGroup = 128; // K of a B stage: one scale group (64-B rows of nibbles)
constexpr int kRowA = 128;  // LDS row bytes, A
constexpr int kRowB = 64;   // LDS row bytes, B
constexpr int kAS = 3;      // A ring slots
constexpr int kBS = 2;      // B ring slots
constexpr int kBBytes = kBN * kRowB;
constexpr int kBGL = kBBytes / (kThreads * 16);  // B DMA instructions per thread per stage (2)
constexpr int kLdsBytes = 160 * 1024;
// groups whose scales fit beside the largest rings (BM 128, two planes)
constexpr int kMaxGroups = (kLdsBytes - kAS * 2 * 128 * kRowA - kBS * kBBytes) / (kBN * 2);

// gemm2's LDS image swizzle (A): 16-B chunk c of 128-B row r is stored at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int swz_a(int b) { return b ^ (((b >> 8) & 7) << 4); }
// B: 16-B chunk c of 64-B row r is stored at chunk c ^ ((r >> 2) & 3)
__device__ __forceinline__ int swz_b(int b) { return b ^ (((b >> 8) & 3) << 4); }

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

// 8 nibbles (k ascending: byte i holds k = 2 i, 2 i + 1) -> one h8 fragment, exactly. mask =
// 0x00F0000F in an SGPR and magic = 0x54006400 in a VGPR: a gfx9 VOP3 takes no literal and one
// scalar operand, so hipcc splits (y & literal) | literal into v_and + v_or; the asm keeps it one
__device__ __forceinline__ h8 cvt8(uint32_t x, uint32_t mask, uint32_t magic) {
    union { h8 v; uint32_t u[4]; } o;
    const h2 bias = {(_Float16)-1032.0f, (_Float16)-72.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        union { uint32_t u; h2 h; } d;
        const uint32_t y = __builtin_amdgcn_perm(x, x, 0x01010101u * i);  // byte i in bytes 0 and 2
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d.u) : "v"(y), "s"(mask), "v"(magic));  // (1024 + n_lo, 64 + n_hi)
        d.h += bias;
        o.u[i] = d.u;
    }
    return o.v;
}

template <int BM, int P, int EPI>
__global__ __launch_bounds__(kThreads) void gemm_w4_kernel(GemmW4Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int A_BYTES = BM * kRowA;  // one plane of one A stage
    constexpr int A_STAGE = P * A_BYTES;
    constexpr int A_GL = A_BYTES / (kThreads * 16);  // DMA instructions per thread per plane
    constexpr int GO = P * A_GL;                     // an odd group: the A stage alone
    constexpr int GE = GO + kBGL;                    // an even group: A and B
    constexpr int B_BASE = kAS * A_STAGE;
    constexpr int S_BASE = B_BASE + kBS * kBBytes;   // scales: [groups][128] fp16
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
    const int K = a.k / S;  // this slice's K extent, from k_begin: whole groups
    const int k_begin = slice * K;
    const int G = K / kGroup, GT = a.k / kGroup;

    // per-thread DMA sources: instruction j of this thread fills LDS bytes j * 4096 + 16 t
    // (lane-linear); that slot holds logical byte swz(.) of the tile
    const char* a_src[P][A_GL];
    const char* b_src[kBGL];
#pragma unroll
    for (int j = 0; j < A_GL; ++j) {
        const int b = swz_a(j * kThreads * 16 + t * 16);
        const int row = min(m0 + (b >> 7), a.m - 1);
#pragma unroll
        for (int p = 0; p < P; ++p)
            a_src[p][j] = reinterpret_cast<const char*>(a.a[p]) + ((size_t)row * a.lda + k_begin) * 2 + (b & 127);
    }
#pragma unroll
    for (int j = 0; j < kBGL; ++j) {
        const int b = swz_b(j * kThreads * 16 + t * 16);
        const int src = b_src_row(EPI, n0, b >> 6, a.pair_off);
        b_src[j] = reinterpret_cast<const char*>(a.w) + ((size_t)src * a.k + k_begin) / 2 + (b & 63);
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
            for (int j = 0; j < kBGL; ++j) glds16(b_src[j] + (size_t)(g >> 1) * kRowB, bb + j * kThreads * 16);
        }
    };

    f4 acc[MI][4], gacc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = gacc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    const uint32_t nib = 0x00F0000Fu, magic = 0x54006400u;  // cvt8's constants
    // one A step: half h (0 / 1) of the group in B slot sb against A slot sa. h == 0 starts the
    // group accumulators from zero.
    auto step = [&](int sa, int sb, int h) {
        const char* As = lds + sa * A_STAGE;
        const char* Bs = lds + B_BASE + sb * kBBytes;
        u32x2 raw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            raw[j] = *reinterpret_cast<const u32x2*>(Bs + swz_b((wc * 64 + j * 16 + fr) * kRowB + 32 * h + 8 * fq));
        h8 af[MI][P][2];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ab = swz_a((wr * (BM / 2) + i * 16 + fr) * kRowA + (2 * fq + u) * 16);
#pragma unroll
                for (int p = 0; p < P; ++p) af[i][p][u] = *reinterpret_cast<const h8*>(As + p * A_BYTES + ab);
            }
        h8 bf[2][2];
        bf[0][0] = cvt8(raw[0][0], nib, magic);
        bf[0][1] = cvt8(raw[0][1], nib, magic);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < 3) {  // among fragment j's MFMAs
                bf[(j + 1) & 1][0] = cvt8(raw[j + 1][0], nib, magic);
                bf[(j + 1) & 1][1] = cvt8(raw[j + 1][1], nib, magic);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const f4 c = (h == 0 && p == 0 && u == 0) ? f4{0.f, 0.f, 0.f, 0.f} : gacc[i][j];
                        gacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][p][u], bf[j & 1][u], c, 0, 0, 0);
                    }
        }
    };

    const int KT = K / kBKA;  // even, >= 2
    issue(0, 0, 0, true);
    issue(1, 1, 0, false);
    // the tile's scales, [G][128] fp16 by tile row (the gate/up pairing included), behind the
    // first two DMA groups; published by the barrier below
    {
        uint16_t* sl = reinterpret_cast<uint16_t*>(lds + S_BASE);
        const int tr = t & 127;
        const uint16_t* src =
            reinterpret_cast<const uint16_t*>(a.scales) + (size_t)b_src_row(EPI, n0, tr, a.pair_off) * GT + k_begin / kGroup;
        for (int g = t >> 7; g < G; g += 2) sl[g * kBN + tr] = src[g];
    }
    __syncthreads();
    const _Float16* sl = reinterpret_cast<const _Float16*>(lds + S_BASE) + wc * 64 + fr;
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
        // the group's sum enters the main accumulator under its scale, in fp32
        const _Float16* sg = sl + (kt >> 1) * kBN;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = (float)sg[16 * j];
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i][j] += s * gacc[i][j];
        }
        sa = sa2;
    }

    // epilogue: C fragment (i, j) register r is row 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15)
    if (EPI == EPI_SILU_MUL) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int m = m0 + wr * (BM / 2) + 16 * i + 4 * fq + r4;
                if (m >= a.m) continue;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int gc = n0 + 32 * wc + 16 * j + fr;
                    const float v = silu_f(acc[i][j][r4]) * acc[i][j + 2][r4];
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
        float* ybase = EPI == EPI_SLAB ? a.slab + (size_t)slice * a.m * a.ldy : a.y;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int m = m0 + wr * (BM / 2) + 16 * i + 4 * fq + r4;
                if (m >= a.m) continue;
                float* yrow = ybase + (size_t)m * a.ldy;
#pragma unroll
                for (int j = 0; j < 4; ++j) yrow[n0 + wc * 64 + 16 * j + fr] = acc[i][j][r4];
            }
    }
}

template <int BM, int P, int EPI>
int launch3(const GemmW4Args& a, int grid, hipStream_t s) {
    constexpr size_t rings = (size_t)kAS * P * BM * kRowA + (size_t)kBS * kBBytes;
    static const bool attr = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w4_kernel<BM, P, EPI>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes) == hipSuccess;
    }();
    LLMI_REQUIRE(attr, "gemm_w4: cannot raise the dynamic LDS limit");
    const size_t lds = rings + (size_t)(a.k / a.ksplit / kGroup) * kBN * 2;
    hipLaunchKernelGGL((gemm_w4_kernel<BM, P, EPI>), dim3(grid), dim3(kThreads), lds, s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

template <int BM, int P>
int launch2(const GemmW4Args& a, int grid, hipStream_t s) {
    switch (a.epi) {
        case EPI_STORE: return launch3<BM, P, EPI_STORE>(a, grid, s);
        case EPI_SILU_MUL: return launch3<BM, P, EPI_SILU_MUL>(a, grid, s);
        default: return launch3<BM, P, EPI_SLAB>(a, grid, s);
    }
}

}  // namespace

bool gemm_w4_supported(int n, int k, int epi, int ksplit) {
    if (epi != EPI_STORE && epi != EPI_SLAB && epi != EPI_SILU_MUL) return false;
    const int ncols = (epi == EPI_SILU_MUL) ? n / 2 : n;
    const int tile = (epi == EPI_SILU_MUL) ? kBN / 2 : kBN;
    const int ks = epi == EPI_SLAB ? ksplit : 1;
    return n > 0 && k > 0 && ks >= 1 && ncols % tile == 0 && (epi != EPI_SILU_MUL || n % 2 == 0) &&
           k % (ks * kGroup) == 0 && k / (ks * kGroup) <= kMaxGroups;
}

int gemm_w4_launch(GemmW4Args a, hipStream_t s) {
    LLMI_REQUIRE(a.a[0] && a.w && a.m > 0, "gemm_w4: null operand or empty M");
    LLMI_REQUIRE(a.scales != nullptr, "gemm_w4: int4 weights need per-group scales");
    LLMI_REQUIRE(a.planes == 1 || (a.planes == 2 && a.a[1]), "gemm_w4: planes must be 1 or 2 (with a[1])");
    if (!gemm_w4_supported(a.n, a.k, a.epi, a.ksplit)) {
        set_last_error("[llmi][ERROR] gemm_w4: store, slab or silu_mul; N a multiple of 128 (gate_up: 2 x 64), "
                       "K / ksplit a multiple of 128, at most 24576");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_REQUIRE(a.epi == EPI_SILU_MUL ? (a.y || a.y_hi) : a.epi == EPI_SLAB ? a.slab != nullptr : a.y != nullptr,
                 "gemm_w4: null output");
    LLMI_REQUIRE(a.lda >= a.k && a.lda % 8 == 0 && (reinterpret_cast<uintptr_t>(a.a[0]) & 15) == 0 &&
                     (a.planes == 1 || (reinterpret_cast<uintptr_t>(a.a[1]) & 15) == 0),
                 "gemm_w4: A planes must be 16-B aligned with lda >= k, lda % 8 == 0");
    LLMI_REQUIRE((reinterpret_cast<uintptr_t>(a.w) & 15) == 0, "gemm_w4: W must be 16-B aligned");
    LLMI_REQUIRE(a.epi != EPI_SILU_MUL || a.pair_off == a.n / 2, "gemm_w4: gate_up pair offset must be N / 2");
    const int ncols = (a.epi == EPI_SILU_MUL) ? a.n / 2 : a.n;
    LLMI_REQUIRE(a.ldy >= ncols, "gemm_w4: ldy must cover the output columns");
    a.n_tiles = ncols / ((a.epi == EPI_SILU_MUL) ? kBN / 2 : kBN);
    if (a.epi != EPI_SLAB) a.ksplit = 1;
    // 128-row tiles unless that leaves CUs idle (gemm_w8's rule; split-K supplies the workgroups)
    const int bm = a.epi == EPI_SLAB || ((a.m + 127) / 128) * a.n_tiles >= 256 ? 128 : 64;
    const int grid = ((a.m + bm - 1) / bm) * a.n_tiles * a.ksplit;
    if (bm == 128) return a.planes == 2 ? launch2<128, 2>(a, grid, s) : launch2<128, 1>(a, grid, s);
    return a.planes == 2 ? launch2<64, 2>(a, grid, s) : launch2<64, 1>(a, grid, s);
}

}  // namespace llmi
