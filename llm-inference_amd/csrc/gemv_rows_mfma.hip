// Multi-row weight-streaming GEMV on the matrix cores: Y[i] = W x_i for m = 1..8 activation
// rows in ONE launch at every k, W [n_rows, k] row-major fp16 or int8 + row scale (DESIGN.md §3
// "Batched decode on the matrix cores"). Opt-in (Batch::set_option "rows_mfma"): faithful to
// fp32 (two fp16 planes of x), not bitwise gemv_launch's.
//
// One v_mfma_f32_16x16x32_f16 takes 16 weight rows x 32 k (A) against 16 activation columns
// (B): columns 0..7 are hi = fp16(v) of sequences 0..7, columns 8..15 lo = fp16(v - hi), with
// v = x * gamma (or plain x); unused sequences are zero columns. Column i + 8 of the fp32 C
// tile is added to column i once per tile (a DPP row rotation), then * rstd, * row scale and
// the epilogue, so sequence i's result depends on column i of B alone.
//
// Split. A 512-thread workgroup owns a 16-row weight tile at a time (gate_up: a gate tile and
// its up tile, the same row offsets) and its 8 waves split K into 8 contiguous slices. A wave
// keeps the B fragments of its slice resident in registers for the whole launch (4 VGPRs per
// 32 k: 64 registers at k = 4096, 216 at k = 13824; built once through a 4 KiB LDS segment per
// wave, see the prologue), so no x image lives in LDS and the weights
// go global -> VGPR -> MFMA: a lane's A operand is the 16-byte chunk it loads (int8: one chunk
// converted in registers to two A operands, exact). Lane (row r = lane % 16, q = lane / 16)
// loads chunk 4 s + q of row r in load step s, so one load instruction reads 64 contiguous
// bytes of each of 16 rows and a batch of U = 4 steps whole 128-byte lines; B is built with the
// same (s, q) -> k map, which is all the MFMA needs. The loads of the next batch -- across
// tile boundaries too -- are issued before the current batch's MFMAs (two register buffers).
// Precondition: |x * gamma| (atomic form: |x|) < 65504, or hi is inf and lo NaN (not checked).
// The 8 partial C tiles meet in LDS (8 KiB, gate_up 16: two buffers, one barrier a tile); wave
// (tile index % 8) adds them in wave order 0..7 and runs the epilogue while the others stream on.
//
// Determinism: the MFMA sums a column in a fixed order, the K slices are added in wave order,
// rstd is a fixed-order sum of per-lane fp32 sums of squares, and workgroups meet only through
// int64 atomics, so a sequence's result is the same bits whatever m is, whichever column it
// sits in, whatever the other columns hold, and from run to run.
#include "gemv_impl.h"

namespace llmi {
namespace {

using namespace gemv_detail;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kMW = 8;               // waves of a workgroup: the K slices
constexpr int kMT = kMW * kWave;
constexpr int kTile = 16;            // weight rows of an MFMA tile
enum Form : int { F_STORE = 0, F_SILU = 1, F_ATOMIC = 2 };
// B fragments (32 k each) a wave can hold: the instantiated slice lengths
constexpr int kSteps[] = {8, 16, 20, 32, 44, 54};

// load steps of a batch: the most of 4, 2, 1 that keeps the B fragments (4 NS), the two weight
// buffers (8 T U), the C tiles and 28 registers of addresses and masks (int8: 24 more for the
// converted operands) within the 256 of two waves a SIMD (0: none, the shape is not served)
constexpr int batch_steps(int ns, int t, bool i8) {
    for (int u = 4; u >= 1; u /= 2)
        if (4 * ns + 8 * t * u + 4 * t + (i8 ? 52 : 28) <= 256) return u;
    return 0;
}
constexpr int kSegK = 128;           // k of a staging segment of the activation planes
template <int T>  // A tiles of a group
struct Lds {
    alignas(16) _Float16 pl[kMW][16][kSegK + 8];  // a segment's planes [wave][column][k], rows 16 bytes apart in banks
    float c[2][kMW][T][kTile * 8];  // [buffer][wave][tile of the group][row * 8 + sequence]
    float ss[kMW][8][8];            // sums of squares [wave][lane % 8][sequence]
};

// 8 int8 -> 8 fp16, exact: byte b ^ 0x80 under the exponent byte of fp16 1024 is 1024 + (b + 128)
__device__ __forceinline__ h8 i8x8_to_h8(uint32_t w0, uint32_t w1) {
    const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
    const uint32_t x0 = w0 ^ 0x80808080u, x1 = w1 ^ 0x80808080u;
    const h2 r0 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04010400u)) - bias;
    const h2 r1 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x0, 0x04030402u)) - bias;
    const h2 r2 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04010400u)) - bias;
    const h2 r3 = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, x1, 0x04030402u)) - bias;
    return (h8){r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
}

// pointer of activation row i (a lane-varying i): selects, no dynamic index into the arguments
#define ROW_PTR(field, i, m)                                                                  \
    [&]() {                                                                                   \
        auto v_ = p.row[0].field;                                                             \
        _Pragma("unroll") for (int j_ = 1; j_ < kGemvRowsMax; ++j_)                           \
            v_ = ((i) == j_ && j_ < (m)) ? p.row[j_].field : v_;                              \
        return v_;                                                                            \
    }()

template <bool I8, int NS, int FORM>
__global__ __launch_bounds__(kMT) void rows_mfma_kernel(const GemvRowsArgs p) {
    constexpr bool NORM = FORM != F_ATOMIC;  // fixed-point x with RMSNorm; else a plain fp32 x
    constexpr int T = FORM == F_SILU ? 2 : 1;  // A tiles of a group
    constexpr int CH = I8 ? 16 : 8;          // k of a 16-byte chunk
    constexpr int FP = CH / 8;               // B fragments a load feeds
    constexpr int NL = NS / FP;              // load steps of a wave's slice
    constexpr int U = batch_steps(NS, T, I8);    // load steps a batch (and register buffer)
    static_assert(U >= 1, "the fragments and two weight buffers exceed 256 registers");
    constexpr int NB = (NL + U - 1) / U;
    static_assert(NS % FP == 0, "int8 slices hold whole chunks");
    __shared__ Lds<T> sm;
    const GemvArgs& a = p.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: so are the slice's bounds and masks
    const int col = lane & 15, q = lane >> 4;
    const int S = FORM == F_ATOMIC ? a.ksplit : 1;
    const int bid0 = blockIdx.x, nblk0 = gridDim.x;
    const int ks = bid0 % S, bid = bid0 / S, nblk = nblk0 / S;
    const int k = a.k / S;                   // this workgroup's K extent
    const int nc = k / CH;                   // chunks of a row
    const int LS = (nc + 3) / 4, LSw = (LS + kMW - 1) / kMW;
    const int s0 = wave * LSw;               // this wave's load steps [s0, s0 + nsw)
    const int nsw = max(0, min(LSw, LS - s0));
    const int cbase = 4 * s0 + q;            // the lane's chunk in load step s0
    const int n_groups = ((FORM == F_SILU ? a.pair_off : a.n_rows) + kTile - 1) / kTile;
    const size_t row_bytes = (size_t)a.k * (I8 ? 1 : 2);
    const char* wbase = reinterpret_cast<const char*>(a.w) + (size_t)ks * k * (I8 ? 1 : 2);

    // branch-free stream as gemv_body's: clamped addresses, masked values
    auto load = [&](uint4 (&wv)[T][U], int g, int b, int cb) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int gr = kTile * g + col;
            const int row = gr + t * a.pair_off;
            const bool rok = FORM == F_SILU ? (gr < a.pair_off && row < a.n_rows) : row < a.n_rows;
            const char* rp = wbase + (size_t)(rok ? row : 0) * row_bytes;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ul = b * U + u;
                if (ul >= NL) continue;
                const int c = cb + 4 * ul;
                uint4 v = ld_nt16(rp + (size_t)min(c, nc - 1) * 16);
                const unsigned m = (rok && ul < nsw && c < nc) ? 0xFFFFFFFFu : 0u;
                v.x &= m; v.y &= m; v.z &= m; v.w &= m;
                wv[t][u] = v;
            }
        }
    };
    uint4 cur[T][U];
    load(cur, bid, 0, cbase);  // in flight while the B fragments are built

    // ---- B fragments of this wave's slice: column col is sequence col % 8, hi (col < 8) or lo.
    // Staged through LDS in segments of kSegK k: the wave's lanes convert the segment of all 8
    // sequences in a rolled loop (lane: sequence lane / 8, four k at a time, so few registers are
    // live whatever the slice length), then each lane reads its fragments with one 16-byte LDS
    // load each, straight into the registers that hold them for the rest of the launch.
    const bool lo = col >= 8;
    h8 bf[NS];
    {
        constexpr int PB = kSegK / (4 * CH);  // load steps a segment
        const int ps = lane >> 3, part = lane & 7;
        const bool live = ps < p.m;
        const long long* xf = ROW_PTR(x_fixed, ps, p.m);
        const float* xr = ROW_PTR(x, ps, p.m);
        float* xo = ROW_PTR(x_out, ps, p.m);
        const int kend = min(4 * (s0 + nsw) * CH, k);  // the slice's end (an idle wave: its start)
        float ss = 0.f;
#pragma unroll
        for (int j0 = 0; j0 < NL; j0 += PB) {
            const int kseg = 4 * (s0 + j0) * CH;
#pragma unroll 1
            for (int e = 0; e < kSegK / 32; ++e) {
                const int kl = 4 * (8 * e + part), kg = kseg + kl;
                const bool ok = live && kg < kend;
                const int ka = min(kg, k - 4);  // clamped address, masked value
                float4 v;
                if constexpr (NORM) {
                    const longlong2 f0 = *reinterpret_cast<const longlong2*>(xf + ka);
                    const longlong2 f1 = *reinterpret_cast<const longlong2*>(xf + ka + 2);
                    v = make_float4(from_fixed(f0.x), from_fixed(f0.y), from_fixed(f1.x), from_fixed(f1.y));
                    if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (bid0 == 0 && xo != nullptr && ok) *reinterpret_cast<float4*>(xo + kg) = v;
                    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
                    const float4 g4 = a.g_dtype == LLMI_F16 ? gamma4<__half>(a.gamma, ka / 4) : gamma4<float>(a.gamma, ka / 4);
                    v.x *= g4.x; v.y *= g4.y; v.z *= g4.z; v.w *= g4.w;
                } else {
                    v = *reinterpret_cast<const float4*>(xr + (size_t)ks * k + ka);
                    if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                const h4 hi = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
                const h4 lw = {(_Float16)(v.x - (float)hi[0]), (_Float16)(v.y - (float)hi[1]),
                               (_Float16)(v.z - (float)hi[2]), (_Float16)(v.w - (float)hi[3])};
                *reinterpret_cast<h4*>(&sm.pl[wave][ps][kl]) = hi;
                *reinterpret_cast<h4*>(&sm.pl[wave][ps + 8][kl]) = lw;
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < PB; ++n)
#pragma unroll
                for (int f = 0; f < FP; ++f)
                    if (j0 + n < NL) bf[(j0 + n) * FP + f] = *reinterpret_cast<const h8*>(&sm.pl[wave][col][(4 * n + q) * CH + 8 * f]);
            __syncthreads();
        }
        if (NORM) sm.ss[wave][part][ps] = ss;
    }
    // residual hand-over, one slice per workgroup and row
#pragma unroll
    for (int i = 0; i < kGemvRowsMax; ++i) {
        if (i >= p.m || p.row[i].seed_dst == nullptr) continue;
        const int per = (a.seed_n + nblk0 - 1) / nblk0;
        const int i0 = bid0 * per, i1 = min(i0 + per, a.seed_n);
        for (int e = i0 + tid; e < i1; e += kMT) p.row[i].seed_dst[e] = a.seed_keep ? p.row[i].seed_src[e] : 0ll;
    }
    __syncthreads();
    float rstd = 1.f;  // of sequence lane % 8 (the epilogue's column)
    if constexpr (NORM) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kMW; ++w)
#pragma unroll
            for (int j = 0; j < 8; ++j) t += sm.ss[w][j][lane & 7];
        rstd = 1.0f / sqrtf(t / (float)k + a.eps);
    }

    auto mma = [&](const uint4 (&wv)[T][U], int b, f4 (&acc)[T]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ul = b * U + u;
            if (ul >= NL) continue;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint4& w = wv[t][u];
                if constexpr (I8) {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(i8x8_to_h8(w.x, w.y), bf[2 * ul], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(i8x8_to_h8(w.z, w.w), bf[2 * ul + 1], acc[t], 0, 0, 0);
                } else {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, w), bf[ul], acc[t], 0, 0, 0);
                }
            }
        }
    };
    // the reducing wave: lane handles outputs o = lane, lane + 64 of the tile's 16 rows x 8
    // sequences (row o / 8, sequence o % 8 = lane % 8), the K slices added in wave order
    auto epilogue = [&](int g, int buf) {
        const int c8 = lane & 7;
        if (c8 >= p.m) return;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = lane + 64 * h;
            const int gr = kTile * g + (o >> 3);
            float sum[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                float s = sm.c[buf][0][t][o];
#pragma unroll
                for (int w = 1; w < kMW; ++w) s += sm.c[buf][w][t][o];
                sum[t] = s * rstd;
            }
            if (gr >= (FORM == F_SILU ? a.pair_off : a.n_rows)) continue;
            if (a.scales != nullptr) {
#pragma unroll
                for (int t = 0; t < T; ++t) sum[t] *= __half2float(a.scales[min(gr + t * a.pair_off, a.n_rows - 1)]);
            }
            if constexpr (FORM == F_SILU) {
                ROW_PTR(y, c8, p.m)[gr] = silu(sum[0]) * sum[1];
            } else if constexpr (FORM == F_STORE) {
                ROW_PTR(y, c8, p.m)[gr] = sum[0];
            } else {
                long long* yacc = ROW_PTR(yacc, c8, p.m);
                if (a.yacc_single) {  // one producer a row: base + fixed(v), written through
                    const long long* base = ROW_PTR(yacc_base, c8, p.m);
                    long long* copy = ROW_PTR(yacc_copy, c8, p.m);
                    const long long b = base ? base[gr] : 0ll;
                    const unsigned long long nv = (unsigned long long)(b + to_fixed(sum[0]));
                    __hip_atomic_store(reinterpret_cast<unsigned long long*>(yacc + gr), nv, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                    if (copy)  // (may be the base: this lane read its row above)
                        __hip_atomic_store(reinterpret_cast<unsigned long long*>(copy + gr), nv, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    atomicAdd(reinterpret_cast<unsigned long long*>(yacc + gr), (unsigned long long)to_fixed(sum[0]));
                }
            }
        }
    };

    // ---- the stream: every wave runs the same tiles (one barrier each), its own K slice
    int it = 0;
    for (int g = bid; g < n_groups; g += nblk, ++it) {
        f4 acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = (f4){0.f, 0.f, 0.f, 0.f};
        const int gn = g + nblk < n_groups ? g + nblk : g;  // (past the end: a re-load, never used)
        // the chunk offsets are the same for every tile: opaque here, or they are hoisted out of the
        // tile loop, one live register pair per load step
        int cb = cbase;
        asm volatile("" : "+v"(cb));
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            uint4 nxt[T][U];
            if (b + 1 < NB) load(nxt, g, b + 1, cb);
            else load(nxt, gn, 0, cb);
            mma(cur, b, acc);
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) cur[t][u] = nxt[t][u];
            // the unrolled batches are one basic block: without a fence the scheduler hoists every
            // later batch's loads to the top and spills the fragments
            __builtin_amdgcn_sched_barrier(0);
        }
        // lo column + hi column, then this slice's partial tile to LDS: lane (col, q) holds
        // rows 4 q .. 4 q + 3 of column col
        const int buf = it & 1;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[t][r] + row_ror<8>(acc[t][r]);
                if (!lo) sm.c[buf][wave][t][(4 * q + r) * 8 + col] = v;
            }
        __syncthreads();
        if (wave == (it & (kMW - 1))) epilogue(g, buf);
    }
}

const char* why_not(const GemvRowsArgs& p, int* steps) {
    const GemvArgs& a = p.a;
    if (p.m < 1 || p.m > kGemvRowsMax) return "m must be 1..8";
    if (a.w_dtype != LLMI_F16 && a.w_dtype != LLMI_I8) return "fp16 and int8 weights only";
    if (a.kpar > 1) return "kpar > 1 is a single-row form";
    if (a.y_tag != nullptr) return "granule rows are a single-row form";
    if (a.xt.buf != nullptr) return "a fused exchange tail is a single-row form";
    if (a.stamps != nullptr) return "no workgroup stamps";
    if (a.ldw != 0 && a.ldw != a.k) return "no row stride (ldw)";
    if (a.w == nullptr || a.n_rows < 1 || a.k < 32) return "no weights, rows or k";
    const bool norm = a.epi == EPI_STORE || a.epi == EPI_SILU_MUL;
    if (!norm && a.epi != EPI_ATOMIC) return "store, silu and atomic epilogues only (the lm_head's argmax is not served)";
    const int S = norm ? 1 : a.ksplit;
    if (S < 1 || a.k % S != 0 || (a.k / S) % 32 != 0) return "k (of a K slice) must be a multiple of 32";
    if (!norm && a.yacc_single && S != 1) return "yacc_single needs ksplit 1";
    if (norm && (a.gamma == nullptr || (a.g_dtype != LLMI_F16 && a.g_dtype != LLMI_F32)))
        return "a fixed-point x comes with an fp16 or fp32 RMSNorm gamma";
    if (!norm && a.gamma != nullptr) return "an fp32 x comes without RMSNorm";
    if (a.epi == EPI_SILU_MUL && (a.pair_off < 1 || a.pair_off >= a.n_rows)) return "pair_off must be in [1, n_rows)";
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(a.w) || !al16(a.gamma)) return "weights and gamma must be 16-byte aligned";
    for (int i = 0; i < p.m; ++i) {
        const GemvRow& r = p.row[i];
        if (norm ? (r.x_fixed == nullptr || r.y == nullptr) : (r.x == nullptr || r.x_fixed != nullptr || r.yacc == nullptr))
            return "x is either fixed point with rmsnorm and a store / silu epilogue, or fp32 with the atomic one";
        if (!al16(r.x_fixed) || !al16(r.x) || !al16(r.x_out)) return "x must be 16-byte aligned";
        if (r.seed_dst != nullptr && a.seed_keep && r.seed_src == nullptr) return "seed_dst without seed_src";
    }
    // B fragments of a wave's slice: ceil(load steps / 8) loads of 1 (fp16) or 2 (int8) fragments
    const int ch = a.w_dtype == LLMI_I8 ? 16 : 8;
    const int ls = (a.k / S / ch + 3) / 4;
    const int need = (ls + kMW - 1) / kMW * (ch / 8);
    for (int ns : kSteps)
        if (need <= ns) {
            if (batch_steps(ns, a.epi == EPI_SILU_MUL ? 2 : 1, ch == 16) < 1) break;
            if (steps) *steps = ns;
            return nullptr;
        }
    return "k too large for register-resident activations (k of a slice <= 13824 fp16, 11264 int8 and silu)";
}

// (both counts below are of the first device that launches: a process's devices are alike; the
// initialisers of function-local statics run once, whichever thread comes first)
int device_cus() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            n = 0;
        return n;
    }();
    return cus;
}

template <bool I8, int NS, int FORM>
int launch_k_(const GemvRowsArgs& p, hipStream_t s);

template <bool I8, int NS, int FORM>
int launch_k(const GemvRowsArgs& p, hipStream_t s) {
    if constexpr (batch_steps(NS, FORM == F_SILU ? 2 : 1, I8) < 1) return LLMI_EUNSUPPORTED;  // (why_not refused it)
    else return launch_k_<I8, NS, FORM>(p, s);
}

template <bool I8, int NS, int FORM>
int launch_k_(const GemvRowsArgs& p, hipStream_t s) {
    auto kern = rows_mfma_kernel<I8, NS, FORM>;
    const GemvArgs& a = p.a;
    static const int resident = [&] {  // workgroups the device holds at once
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kern), kMT, 0) != hipSuccess)
            n = 0;
        return n * device_cus();
    }();
    const int S = FORM == F_ATOMIC ? a.ksplit : 1;
    const int groups = ((FORM == F_SILU ? a.pair_off : a.n_rows) + kTile - 1) / kTile;
    int nblk = groups;
    if (a.grid > 0) nblk = std::min(nblk, std::max(1, a.grid / S));
    else if (resident >= S) nblk = std::min(nblk, resident / S);
    hipLaunchKernelGGL(kern, dim3(nblk * S), dim3(kMT), 0, s, p);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

template <bool I8, int NS>
int launch_form(const GemvRowsArgs& p, hipStream_t s) {
    switch (p.a.epi) {
        case EPI_STORE: return launch_k<I8, NS, F_STORE>(p, s);
        case EPI_SILU_MUL: return launch_k<I8, NS, F_SILU>(p, s);
        default: return launch_k<I8, NS, F_ATOMIC>(p, s);
    }
}

template <bool I8>
int launch_steps(const GemvRowsArgs& p, int ns, hipStream_t s) {
    switch (ns) {
        case 8: return launch_form<I8, 8>(p, s);
        case 16: return launch_form<I8, 16>(p, s);
        case 20: return launch_form<I8, 20>(p, s);
        case 32: return launch_form<I8, 32>(p, s);
        case 44: return launch_form<I8, 44>(p, s);
        case 54: return launch_form<I8, 54>(p, s);
    }
    return LLMI_EINVAL;
}

}  // namespace

bool gemv_rows_mfma_supported(const GemvRowsArgs& p) { return why_not(p, nullptr) == nullptr; }

int gemv_rows_mfma_launch(const GemvRowsArgs& p, hipStream_t s) {
    int ns = 0;
    if (const char* why = why_not(p, &ns)) {
        set_last_error(std::string("[llmi][ERROR] gemv_rows_mfma: ") + why);
        return LLMI_EUNSUPPORTED;
    }
    return p.a.w_dtype == LLMI_I8 ? launch_steps<true>(p, ns, s) : launch_steps<false>(p, ns, s);
}

}  // namespace llmi
