// Multi-row streaming GEMV body (gemv_rows.hip has the design notes; gemv_rows_launch.h the
// kernel and its launchers).
//
// The body is gemv_body (gemv_impl.h) with M x images in LDS and M accumulators per weight
// row: the same 256-thread workgroup, the same row groups per wave, the same chunks
// lane, lane + 64, ... in ascending order per (weight row, activation row), then the same
// wave_sum, * rstd, * scale and epilogue. The unroll only sets how many loads are in flight.
#pragma once
#include "gemv_impl.h"

namespace llmi {
namespace gemv_detail {

#ifndef LLMI_ROWS_UNROLL
#define LLMI_ROWS_UNROLL 4  // 16-B loads per weight row and buffer in flight per lane
#endif
#ifndef LLMI_ROWS_MAX_LDS
#define LLMI_ROWS_MAX_LDS (160 * 1024)  // a workgroup may take the CU's whole LDS
#endif
constexpr int kRowsUnroll = LLMI_ROWS_UNROLL;
constexpr int kRowsStage = 4;  // float4s of every x row a thread holds in registers while staging

// LDS of an m-row launch: [m][PK][nc] float4 images, reduction scratch, [m][waves] argmax keys
__host__ __device__ inline size_t gemv_rows_lds_bytes(int k, int m) {
    return (size_t)m * k * 4 + 16 * 4 + (size_t)m * kWavesPerBlock * 8;
}

// ss + (x^2 + y^2 + z^2 + w^2) with every product and sum rounded on its own, left to right:
// what gemv_body's `ss += v.x * v.x + ...` compiles to (packed multiplies, then scalar adds).
// Written out with contraction off because here the compiler would otherwise fuse some of the
// products into FMAs (it pairs the rows' squares differently), which moves rstd by an ulp.
__device__ __forceinline__ float sumsq4(float ss, const float4& v) {
#pragma clang fp contract(off)
    const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z, ww = v.w * v.w;
    const float t = ((xx + yy) + zz) + ww;
    return ss + t;
}

template <typename WT, int ROWS, int EPI, bool NORM, typename GT, int kUnroll, bool XFIX, int M>
__device__ __forceinline__ void gemv_rows_body(const GemvRowsArgs& p, int bid, int nblk, float4* xs) {
    using IO = PlainIO;
    const GemvArgs& a = p.a;
    constexpr int EPL = WT_<WT>::EPL;
    constexpr int PK = EPL / 4;
    static_assert(!(XFIX && EPI == EPI_ATOMIC), "split-K reads an fp32 x");
    const int bid0 = bid, nblk0 = nblk;
    const int S = (EPI == EPI_ATOMIC) ? a.ksplit : 1;
    const int ks = bid % S;
    bid /= S;
    nblk /= S;
    const int k = a.k / S;
    const int k4 = k / 4;
    const int nc = k / EPL;
    float* red = reinterpret_cast<float*>(xs + (size_t)M * k4);
    unsigned long long* best_s = reinterpret_cast<unsigned long long*>(red + 16);  // [M][waves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_groups = (EPI == EPI_SILU_MUL) ? a.pair_off : (a.n_rows + ROWS - 1) / ROWS;
    const size_t row_bytes = (size_t)(a.ldw ? a.ldw : a.k) * sizeof(WT);
    const char* wbase = reinterpret_cast<const char*>(a.w) + (size_t)ks * k * sizeof(WT);

    auto rows_of = [&](int g, int* rows) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) rows[r] = (EPI == EPI_SILU_MUL) ? g + r * a.pair_off : g * ROWS + r;
    };
    // branch-free stream as gemv_body's: clamped addresses, masked values
    auto load_batch = [&](uint4 (&wv)[ROWS][kUnroll], const int* rows, int base) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int c = base + u * kWave + lane;
            const int cc = c < nc ? c : nc - 1;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int rr = rows[r] < a.n_rows ? rows[r] : a.n_rows - 1;
                const unsigned m = (c < nc && rows[r] < a.n_rows) ? 0xFFFFFFFFu : 0u;
                uint4 v = ld_nt16(wbase + (size_t)rr * row_bytes + (size_t)cc * 16);
                v.x &= m; v.y &= m; v.z &= m; v.w &= m;
                wv[r][u] = v;
            }
        }
    };
    // one weight chunk against the M images: the x packets of image i are read once for the
    // ROWS weight rows of the group
    auto dot_batch = [&](const uint4 (&wv)[ROWS][kUnroll], int base, float (&acc)[ROWS][M]) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int c = base + u * kWave + lane;
            const float4* xp = xs + (c < nc ? c : nc - 1);
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
                    acc[r][i] += dot_packet(wv[r][u], xp + (size_t)i * k4, nc, (WT*)nullptr);
        }
    };

    // ---- prologue: every row's x loads of a staging batch are issued together, then this
    // wave's first weight batch, then the images are written (thread t takes float4s
    // t, t + 256, ... of every row in ascending order: gemv_body's sum-of-squares order)
    const int g0 = bid * kWavesPerBlock + wave;
    int rows0[ROWS];
    rows_of(g0, rows0);
    uint4 w0[ROWS][kUnroll];
    float ss[M];
#pragma unroll
    for (int i = 0; i < M; ++i) ss[i] = 0.f;
    for (int j0 = 0; j0 < k4; j0 += kRowsStage * kThreads) {
        float4 xv[XFIX ? 1 : M][kRowsStage], gv[kRowsStage];
        longlong2 xf[XFIX ? M : 1][kRowsStage][2];
#pragma unroll
        for (int t = 0; t < kRowsStage; ++t) {
            int j = j0 + tid + t * kThreads;
            j = j < k4 ? j : k4 - 1;
            if (NORM) gv[t] = gamma4<GT>(a.gamma, j);
#pragma unroll
            for (int i = 0; i < M; ++i) {
                if constexpr (XFIX) {
                    xf[i][t][0] = IO::ld_ll2(reinterpret_cast<const longlong2*>(p.row[i].x_fixed) + 2 * j);
                    xf[i][t][1] = IO::ld_ll2(reinterpret_cast<const longlong2*>(p.row[i].x_fixed) + 2 * j + 1);
                } else {
                    xv[i][t] = IO::ld4(reinterpret_cast<const float4*>(p.row[i].x + (size_t)ks * k) + j);
                }
            }
        }
        if (j0 == 0) load_batch(w0, rows0, 0);
#pragma unroll
        for (int t = 0; t < kRowsStage; ++t) {
            const int j = j0 + tid + t * kThreads;
            if (j < k4) {
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    float4 v;
                    if constexpr (XFIX) {
                        v = make_float4(from_fixed(xf[i][t][0].x), from_fixed(xf[i][t][0].y),
                                        from_fixed(xf[i][t][1].x), from_fixed(xf[i][t][1].y));
                        if (bid0 == 0 && p.row[i].x_out != nullptr)
                            IO::st4(reinterpret_cast<float4*>(p.row[i].x_out) + j, v);
                    } else {
                        v = xv[i][t];
                    }
                    if (NORM) {
                        ss[i] = sumsq4(ss[i], v);
                        v.x *= gv[t].x; v.y *= gv[t].y; v.z *= gv[t].z; v.w *= gv[t].w;
                    }
                    xs[(size_t)i * k4 + (j % PK) * nc + j / PK] = v;
                }
            }
        }
    }
    // residual hand-over, one slice per workgroup and row
#pragma unroll
    for (int i = 0; i < M; ++i) {
        if (p.row[i].seed_dst == nullptr) continue;
        const int per = (a.seed_n + nblk0 - 1) / nblk0;
        const int i0 = bid0 * per, i1 = min(i0 + per, a.seed_n);
        for (int e = i0 + tid; e < i1; e += kThreads)
            IO::st_ll(p.row[i].seed_dst + e, a.seed_keep ? IO::ld_ll(p.row[i].seed_src + e) : 0ll);
    }
    float rstd[M];
#pragma unroll
    for (int i = 0; i < M; ++i) rstd[i] = 1.f;
    if (NORM) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float t = block_sum(ss[i], red);  // its barriers also publish xs
            rstd[i] = 1.0f / sqrtf(t / (float)k + a.eps);
        }
    } else {
        __syncthreads();
    }

    unsigned long long best[M];
#pragma unroll
    for (int i = 0; i < M; ++i) best[i] = 0ull;

    auto finish = [&](int g, const int* rows, float (&acc)[ROWS][M]) {
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                acc[r][i] = wave_sum(acc[r][i]) * rstd[i];
                if (a.scales != nullptr && rows[r] < a.n_rows) acc[r][i] *= __half2float(a.scales[rows[r]]);
            }
        if (EPI == EPI_SILU_MUL) {
#pragma unroll
            for (int i = 0; i < M; ++i)
                if (lane == i) IO::st(p.row[i].y + g, silu(acc[0][i]) * acc[1][i]);
            return;
        }
        // lane r + ROWS * i writes (weight row r, activation row i)
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = rows[r];
                if (row >= a.n_rows) continue;
                if (lane == r + ROWS * i) {
                    float v = acc[r][i];
                    if (EPI == EPI_ATOMIC) {
                        if (a.yacc_single) {
                            const long long b = p.row[i].yacc_base ? IO::ld_ll(p.row[i].yacc_base + row) : 0ll;
                            const unsigned long long nv = (unsigned long long)(b + to_fixed(v));
                            __hip_atomic_store(reinterpret_cast<unsigned long long*>(p.row[i].yacc + row), nv,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (p.row[i].yacc_copy)  // (may be yacc_base: this lane read its row above)
                                __hip_atomic_store(reinterpret_cast<unsigned long long*>(p.row[i].yacc_copy + row),
                                                   nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        } else {
                            atomicAdd(reinterpret_cast<unsigned long long*>(p.row[i].yacc + row),
                                      (unsigned long long)to_fixed(v));
                        }
                    } else {
                        // gemv_body's `v += resid_scale * resid` compiles to one FMA in every
                        // instantiation; spelled out so that this one cannot come out unfused
                        if (EPI == EPI_ADD) v = fmaf(a.resid_scale, IO::ld(p.row[i].resid + row), v);
                        IO::st(p.row[i].y + row, v);
                    }
                }
                if (EPI == EPI_ARGMAX) {
                    const unsigned long long kk = argmax_key(acc[r][i], a.idx_base + (uint32_t)row);
                    best[i] = kk > best[i] ? kk : best[i];
                }
            }
    };

    // ---- software-pipelined stream over (row group, batch) items: the next item's loads are
    // issued before the current item's convert + FMA work, across row-group boundaries too (two
    // register buffers, manually unrolled by 2 -- gemv_body's PIPE form). With the LDS full a CU
    // holds one workgroup, one wave per SIMD: nothing else hides the load latency. The item
    // after the last one re-loads the last item (a cache hit, never used). A row's batches are
    // still summed in ascending order.
    constexpr int B = kWave * kUnroll;  // chunks per batch
    const int stride = nblk * kWavesPerBlock;
    if (g0 < n_groups) {
        auto advance = [&](int& g, int& base) {
            base += B;
            if (base >= nc) {
                base = 0;
                g += stride;
            }
        };
        float acc[ROWS][M];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int i = 0; i < M; ++i) acc[r][i] = 0.f;
        int ga = g0, ba = 0;
        int rows_a[ROWS], rows_b[ROWS];
        rows_of(ga, rows_a);
        uint4 wb[ROWS][kUnroll];
        auto step = [&](const uint4 (&cur)[ROWS][kUnroll], const int* rows_c, int gc, int bc) {
            dot_batch(cur, bc, acc);
            if (bc + B >= nc) {
                finish(gc, rows_c, acc);
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int i = 0; i < M; ++i) acc[r][i] = 0.f;
            }
        };
        for (;;) {
            int gb = ga, bb = ba;
            advance(gb, bb);
            const bool vb = gb < n_groups;
            if (!vb) { gb = ga; bb = ba; }
            rows_of(gb, rows_b);
            load_batch(wb, rows_b, bb);
            step(w0, rows_a, ga, ba);
            if (!vb) break;
            int gc = gb, bc = bb;
            advance(gc, bc);
            const bool vc = gc < n_groups;
            if (!vc) { gc = gb; bc = bb; }
            rows_of(gc, rows_a);
            load_batch(w0, rows_a, bc);
            step(wb, rows_b, gb, bb);
            if (!vc) break;
            ga = gc;
            ba = bc;
        }
    }
    if (EPI == EPI_ARGMAX) {  // one key per workgroup and activation row, as gemv_body's
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < M; ++i) best_s[i * kWavesPerBlock + wave] = best[i];
        __syncthreads();
        if (tid < M) {
            unsigned long long b = best_s[tid * kWavesPerBlock];
            for (int w = 1; w < kWavesPerBlock; ++w)
                b = best_s[tid * kWavesPerBlock + w] > b ? best_s[tid * kWavesPerBlock + w] : b;
            unsigned long long* dst = p.row[0].partials;
#pragma unroll
            for (int i = 1; i < M; ++i) dst = tid == i ? p.row[i].partials : dst;
            __hip_atomic_store(dst + bid, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

inline int rows_unsupported(const char* what) {
    set_last_error(std::string("[llmi][ERROR] gemv_rows: ") + what);
    return LLMI_EUNSUPPORTED;
}

}  // namespace gemv_detail
}  // namespace llmi
