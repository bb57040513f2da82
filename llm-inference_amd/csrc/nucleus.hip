// Temperature / top-k / top-p / repetition-penalty sampling over a whole logits row
// (llmi_sample_nucleus, llmi_engine_set_sampling_params). The reference has no such
// operator; the rule is this project's own (DESIGN.md "Nucleus sampler"), restated in
// numpy by tests/nucleus_ref.py:
//   z <- penalty (HF rule over the distinct history ids), z <- z / T, NaN -> -inf;
//   order = argmax_key order (value descending, ties to the lower id); m = max z;
//   w_i = rint((double)expf(z_i - m) * 2^32) as uint64 (z_i == m: 2^32 exactly);
//   C = first top_k of the order; P = ceil(top_p * S_C); K = shortest rank prefix of C
//   with weight >= P; R = ceil(u * S_K); result = first id of K, in id order, whose
//   running weight reaches R. Every sum is over integers: exact in any order.
//
// One workgroup of 1024 lanes per row. The row is read once (16-byte loads where the row
// is aligned), turned into 32-bit ordered keys and kept in LDS (vocab <= 32768: 128 KB);
// larger rows (<= 131072) recompute the key from the L2-resident row in every pass. The
// seen-id set is an LDS bitmap. No sort: a cut of the order is (tau, idc) -- keys above
// tau, and of the keys equal to tau the ids <= idc -- found by a descent over the key
// with a 2048-bucket LDS histogram of integer counts or weights (level 0 buckets z
// linearly below the maximum, which spreads a softmax row's bulk over many buckets;
// the next levels split the chosen bucket's own [min, max] key interval by its leading
// bits), then an id-order walk inside the tie group. The draw is the same id-order walk
// over the weights: per-wave totals, then one wave scans its 64-id tiles. LDS integer
// atomics only (order-independent), no global atomics, no cross-workgroup traffic.
#include <vector>

#include "kernels.h"
#include "rowkeys.h"
#include "xorwow.h"

namespace llmi {
namespace {

constexpr int kNucThreads = kRowThreads;
constexpr int kNucWaves = kNucThreads / kWave;
constexpr int kNucBuckets = 2 * kNucThreads;
constexpr int kNucLdsVocab = 32768;      // keys held in LDS up to here
constexpr int kNucMaxVocab = 131072;     // bitmap 16 KB

struct NucArgs {
    const float* logits;
    int vocab;
    const int32_t* history;
    int history_stride;
    const int32_t* history_len;  // null: no history (operator form)
    float penalty, temperature;
    int top_k;
    float top_p;
    uint64_t step;
    int32_t* out_id;
    int32_t* out_kept;
    const uint32_t* jumps;
    // engine form: history = tokens[0 .. cur_pos], step = seed + cur_pos + 1, id -> partials
    const DecodeState* st;
    unsigned long long* partials;
    int np;
};

struct Cut {  // a prefix of the order: key > tau, or key == tau and id <= idc
    uint32_t tau;
    int idc;
};
__device__ __forceinline__ bool in_cut(uint32_t key, int i, Cut c) {
    return key > c.tau || (key == c.tau && i <= c.idc);
}

// scratch at the head of the dynamic LDS region
struct NucScratch {
    unsigned long long red[kNucWaves];
    unsigned long long above;
    uint32_t lo[kNucWaves], hi[kNucWaves];
    int sel, res;
    float u;
    int pad[3];
};

template <bool kLds>
struct Row {
    const float* row;
    const uint32_t* keys;   // LDS (kLds)
    const uint32_t* seen;   // LDS bitmap
    float penalty, temperature;
    bool pen, temp;
    int vocab;
    __device__ __forceinline__ uint32_t make(float z, int i) const {
        if (pen && ((seen[i >> 5] >> (i & 31)) & 1u)) z = z > 0.f ? __fdiv_rn(z, penalty) : __fmul_rn(z, penalty);
        if (temp) z = __fdiv_rn(z, temperature);
        if (z != z) z = -INFINITY;
        return key_of(z);
    }
    __device__ __forceinline__ uint32_t key(int i) const { return kLds ? keys[i] : make(row[i], i); }
};

// sum of the weights and the size of a cut
template <bool kLds>
__device__ void cut_totals(const Row<kLds>& r, Cut c, uint32_t mkey, float m, NucScratch* sc,
                           unsigned long long* sum, int* count) {
    unsigned long long s = 0, n = 0;
    for (int i = threadIdx.x; i < r.vocab; i += kNucThreads) {
        const uint32_t k = r.key(i);
        if (in_cut(k, i, c)) {
            s += weight_of(k, mkey, m);
            n += 1;
        }
    }
    *sum = block_sum_u64(s, sc->red);
    *count = (int)block_sum_u64(n, sc->red);
}

// smallest id whose id-order running sum of q(i) reaches target (>= 1, <= the total)
template <typename Q>
__device__ int id_walk(int vocab, unsigned long long target, int fallback, NucScratch* sc, Q q) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int per = ((vocab + kNucThreads - 1) / kNucThreads) * kWave;  // ids per wave
    const int lo = wid * per, hi = min(vocab, lo + per);
    unsigned long long s = 0;
    for (int i = lo + lane; i < hi; i += kWave) s += q(i);
    s = wave_sum_u64(s);
    __syncthreads();
    if (lane == 0) sc->red[wid] = s;
    if (threadIdx.x == 0) sc->res = fallback;
    __syncthreads();
    unsigned long long run = 0;
    int wsel = -1;
#pragma unroll
    for (int j = 0; j < kNucWaves; ++j) {
        const unsigned long long t = sc->red[j];
        if (wsel < 0) {
            if (run + t >= target) wsel = j;
            else run += t;
        }
    }
    if (wid == wsel) {
        for (int t0 = lo; t0 < hi; t0 += kWave) {
            const int i = t0 + lane;
            const unsigned long long incl = wave_scan_u64(i < hi ? q(i) : 0ull, lane);
            const unsigned long long hit = __ballot(run + incl >= target);
            if (hit) {
                if (lane == __ffsll((long long)hit) - 1) sc->res = i;
                break;
            }
            run += __shfl(incl, kWave - 1, kWave);
        }
    }
    __syncthreads();
    return sc->res;
}

// The cut of `set` at which the rank-order running sum of q (kWeight: the weights, else 1)
// first reaches target: returns the prefix (tau, idc).
template <bool kLds, bool kWeight>
__device__ Cut descend(const Row<kLds>& r, Cut set, unsigned long long target, uint32_t mkey, float m,
                       unsigned long long* hist, NucScratch* sc) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t klo = 0u, khi = 0xFFFFFFFFu;
    unsigned long long above = 0;
    for (int level = 0; level < 6; ++level) {
        int shift = 0;
        if (level > 0) {
            const uint32_t range = khi - klo;
            shift = range < (uint32_t)kNucBuckets ? 0 : (32 - __clz(range)) - 11;
        }
        auto bucket = [&](uint32_t k) -> int {  // 0 = the highest keys
            if (level > 0) return (int)((khi - k) >> shift);
            if (k == mkey) return 0;
            return (int)fminf((m - z_of(k)) * 64.f, (float)(kNucBuckets - 1));
        };
        hist[2 * threadIdx.x] = 0ull;
        hist[2 * threadIdx.x + 1] = 0ull;
        if (threadIdx.x == 0) sc->sel = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < r.vocab; i += kNucThreads) {
            const uint32_t k = r.key(i);
            if (k < klo || k > khi || !in_cut(k, i, set)) continue;
            const unsigned long long q = kWeight ? weight_of(k, mkey, m) : 1ull;
            if (q) atomicAdd(&hist[bucket(k)], q);
        }
        __syncthreads();
        // rank-order scan of the buckets: lane t holds buckets 2t, 2t + 1
        const unsigned long long a = hist[2 * threadIdx.x], b = hist[2 * threadIdx.x + 1];
        unsigned long long incl = wave_scan_u64(a + b, lane);
        if (lane == kWave - 1) sc->red[wid] = incl;
        __syncthreads();
        unsigned long long excl = above + incl - (a + b);
        for (int j = 0; j < wid; ++j) excl += sc->red[j];
        if (excl < target && excl + a + b >= target) {  // exactly one lane
            const bool first = excl + a >= target;
            sc->sel = 2 * (int)threadIdx.x + (first ? 0 : 1);
            sc->above = first ? excl : excl + a;
        }
        __syncthreads();
        const int sel = sc->sel;
        above = sc->above;
        // the chosen bucket's own key interval
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        for (int i = threadIdx.x; i < r.vocab; i += kNucThreads) {
            const uint32_t k = r.key(i);
            if (k < klo || k > khi || !in_cut(k, i, set) || bucket(k) != sel) continue;
            lo = min(lo, k);
            hi = max(hi, k);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor(lo, off, kWave));
            hi = max(hi, (uint32_t)__shfl_xor(hi, off, kWave));
        }
        if (lane == 0) {
            sc->lo[wid] = lo;
            sc->hi[wid] = hi;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kNucWaves; ++j) {
            lo = min(lo, sc->lo[j]);
            hi = max(hi, sc->hi[j]);
        }
        __syncthreads();
        klo = lo;
        khi = hi;
        if (klo >= khi) break;
    }
    // the tie group at tau, in id order: as many of its ids as the remainder needs
    const uint32_t tau = klo;
    unsigned long long need = target - above;
    if (kWeight) {
        const unsigned long long w = weight_of(tau, mkey, m);
        need = w ? (need + w - 1) / w : need;
    }
    Cut c;
    c.tau = tau;
    c.idc = id_walk(r.vocab, need, set.idc < r.vocab ? set.idc : r.vocab - 1, sc, [&](int i) -> unsigned long long {
        return (r.key(i) == tau && in_cut(tau, i, set)) ? 1ull : 0ull;
    });
    return c;
}

template <bool kLds>
__global__ __launch_bounds__(kNucThreads) void nucleus_kernel(NucArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    NucScratch* sc = reinterpret_cast<NucScratch*>(smem);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(smem + 512);
    uint32_t* seen = reinterpret_cast<uint32_t*>(smem + 512 + kNucBuckets * 8);
    const int V = a.vocab;
    const int seen_words = (V + 31) / 32;
    uint32_t* keys = seen + ((seen_words + 3) & ~3);
    const int b = blockIdx.x;
    const float* row = a.logits + (size_t)b * V;

    const int32_t* hist_ids = a.history;
    int n_hist = 0;
    uint64_t step = a.step;
    if (a.st) {
        n_hist = a.st->cur_pos + 1;
        step += (uint64_t)n_hist;
    } else if (a.history_len) {
        n_hist = a.history_len[b];
        hist_ids += (size_t)b * a.history_stride;
    }
    const bool pen = a.penalty != 1.0f && n_hist > 0;
    if (threadIdx.x == 0) {  // the draw: curand_uniform of curand_init(step, row, 0)
        XorwowState rs = xorwow_init(step);
        if (b > 0) xorwow_jump(rs, (uint32_t)b, a.jumps);
        sc->u = xorwow_uniform(xorwow_next(rs));
    }
    if (pen) {
        for (int i = threadIdx.x; i < seen_words; i += kNucThreads) seen[i] = 0u;
        __syncthreads();
        for (int i = threadIdx.x; i < n_hist; i += kNucThreads) {
            const int id = hist_ids[i];
            if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
    }
    Row<kLds> r;
    r.row = row; r.keys = keys; r.seen = seen; r.penalty = a.penalty; r.temperature = a.temperature;
    r.pen = pen; r.temp = a.temperature != 1.0f; r.vocab = V;

    // the row, once: keys into LDS, the maximum key
    uint32_t mk = 0u;
    if (kLds) {
        const int head = min(V, (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u));
        const int nv = (V - head) / 4;
        for (int v = threadIdx.x; v < nv; v += kNucThreads) {
            const int i = head + 4 * v;
            const float4 x = *reinterpret_cast<const float4*>(row + i);
            const uint32_t k0 = r.make(x.x, i), k1 = r.make(x.y, i + 1), k2 = r.make(x.z, i + 2), k3 = r.make(x.w, i + 3);
            keys[i] = k0; keys[i + 1] = k1; keys[i + 2] = k2; keys[i + 3] = k3;
            mk = max(max(mk, k0), max(k1, max(k2, k3)));
        }
        const int rest = V - 4 * nv;  // head + tail elements, scalar
        if ((int)threadIdx.x < rest) {
            const int i = (int)threadIdx.x < head ? (int)threadIdx.x : 4 * nv + (int)threadIdx.x;
            const uint32_t k = r.make(row[i], i);
            keys[i] = k;
            mk = max(mk, k);
        }
    } else {
        for (int i = threadIdx.x; i < V; i += kNucThreads) mk = max(mk, r.key(i));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mk = max(mk, (uint32_t)__shfl_xor(mk, off, kWave));
    if ((threadIdx.x & 63) == 0) sc->lo[threadIdx.x >> 6] = mk;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kNucWaves; ++j) mk = max(mk, sc->lo[j]);
    __syncthreads();
    const uint32_t mkey = mk;
    const float m = z_of(mkey);

    // top-k, then top-p inside it
    Cut cut;
    cut.tau = 0u;
    cut.idc = 0x7FFFFFFF;
    if (a.top_k > 0 && a.top_k < V) cut = descend<kLds, false>(r, cut, (unsigned long long)a.top_k, mkey, m, hist, sc);
    unsigned long long S = 0;
    int kept = 0;
    if (a.top_p < 1.0f) {
        cut_totals(r, cut, mkey, m, sc, &S, &kept);
        unsigned long long P = (unsigned long long)ceil((double)a.top_p * (double)S);
        P = P < 1ull ? 1ull : (P > S ? S : P);
        cut = descend<kLds, true>(r, cut, P, mkey, m, hist, sc);
    }
    cut_totals(r, cut, mkey, m, sc, &S, &kept);
    unsigned long long R = (unsigned long long)ceil((double)sc->u * (double)S);
    R = R < 1ull ? 1ull : (R > S ? S : R);
    // fallback of the walk (never taken for a consistent S): the row's argmax id
    int amax = V;
    for (int i = threadIdx.x; i < V; i += kNucThreads)
        if (r.key(i) == mkey) { amax = i; break; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = min(amax, __shfl_xor(amax, off, kWave));
    if ((threadIdx.x & 63) == 0) sc->lo[threadIdx.x >> 6] = (uint32_t)amax;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kNucWaves; ++j) amax = min(amax, (int)sc->lo[j]);
    if (amax >= V) amax = 0;
    const Cut K = cut;
    const int id = id_walk(V, R, amax, sc, [&](int i) -> unsigned long long {
        const uint32_t k = r.key(i);
        return in_cut(k, i, K) ? weight_of(k, mkey, m) : 0ull;
    });
    if (a.partials) {
        if (threadIdx.x == 0) a.partials[0] = argmax_key(1.0f, (uint32_t)id);
        for (int i = 1 + threadIdx.x; i < a.np; i += kNucThreads) a.partials[i] = 0ull;
    } else if (threadIdx.x == 0) {
        a.out_id[b] = id;
        if (a.out_kept) a.out_kept[b] = kept;
    }
}

size_t nucleus_lds_bytes(int vocab, bool lds) {
    const size_t seen_words = (((size_t)vocab + 31) / 32 + 3) & ~(size_t)3;
    return 512 + (size_t)kNucBuckets * 8 + seen_words * 4 + (lds ? (((size_t)vocab + 3) & ~(size_t)3) * 4 : 0);
}

int nucleus_dispatch(const NucArgs& a, int rows, hipStream_t s) {
    static_assert(sizeof(NucScratch) <= 512, "scratch region");
    const bool lds = a.vocab <= kNucLdsVocab;
    const size_t bytes = nucleus_lds_bytes(a.vocab, lds);
    static const hipError_t attr = [] {  // once: the 160 KiB workgroup LDS (both forms), for every vocab
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nucleus_kernel<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)nucleus_lds_bytes(kNucLdsVocab, true));
        if (e != hipSuccess) return e;
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&nucleus_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)nucleus_lds_bytes(kNucMaxVocab, false));
    }();
    LLMI_HIP(attr);
    if (lds)
        hipLaunchKernelGGL(nucleus_kernel<true>, dim3(rows), dim3(kNucThreads), bytes, s, a);
    else
        hipLaunchKernelGGL(nucleus_kernel<false>, dim3(rows), dim3(kNucThreads), bytes, s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int nucleus_check_params(const char* who, int vocab, float penalty, float temperature, int top_k, float top_p) {
    const std::string w(who);
    LLMI_REQUIRE(temperature > 0.f, w + ": temperature must be > 0 (greedy decoding is top_k = 1)");
    LLMI_REQUIRE(top_p > 0.f && top_p <= 1.f, w + ": top_p must be in (0, 1]");
    LLMI_REQUIRE(penalty > 0.f, w + ": repetition_penalty must be > 0 (1 = none)");
    LLMI_REQUIRE(top_k >= 0, w + ": top_k must be >= 0 (0 = no limit)");
    if (vocab > kNucMaxVocab) {
        set_last_error("[llmi][ERROR] " + w + ": vocab above 131072 is not supported");
        return LLMI_EUNSUPPORTED;
    }
    return LLMI_OK;
}

}  // namespace

int sample_nucleus_launch(const float* logits, int rows, int vocab, const int32_t* history, int history_stride,
                          const int32_t* history_len, float penalty, float temperature, int top_k, float top_p,
                          uint64_t step, int32_t* out_id, int32_t* out_kept, hipStream_t s) {
    LLMI_REQUIRE(logits && out_id, "sample_nucleus: null logits or out_id");
    LLMI_REQUIRE(rows > 0 && vocab > 0, "sample_nucleus: rows and vocab must be positive");
    LLMI_REQUIRE(rows <= (1 << kXorwowJumpBits), "sample_nucleus: at most 65536 rows (curand subsequence jumps)");
    LLMI_REQUIRE(!history_len || (history && history_stride >= 0),
                 "sample_nucleus: history_len without a history (null pointer or negative stride)");
    LLMI_TRY(nucleus_check_params("sample_nucleus", vocab, penalty, temperature, top_k, top_p));
    if (history_len) {
        // ids are checked on the host unless the stream is capturing (no copies inside a
        // capture); the kernel itself skips any id outside [0, vocab)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        LLMI_HIP(hipStreamIsCapturing(s, &cap));
        if (cap == hipStreamCaptureStatusNone) {
            std::vector<int32_t> len(rows), ids;
            LLMI_HIP(hipMemcpyAsync(len.data(), history_len, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
            LLMI_HIP(hipStreamSynchronize(s));
            for (int b = 0; b < rows; ++b) {
                LLMI_REQUIRE(len[b] >= 0 && (rows == 1 || len[b] <= history_stride),
                             "sample_nucleus: history_len must be in [0, history_stride]");
                if (len[b] == 0) continue;
                ids.resize(len[b]);
                LLMI_HIP(hipMemcpyAsync(ids.data(), history + (size_t)b * history_stride, (size_t)len[b] * 4,
                                        hipMemcpyDeviceToHost, s));
                LLMI_HIP(hipStreamSynchronize(s));
                for (int32_t id : ids)
                    LLMI_REQUIRE(id >= 0 && id < vocab, "sample_nucleus: history ids must be in [0, vocab)");
            }
        }
    }
    NucArgs a{};
    a.logits = logits; a.vocab = vocab; a.history = history; a.history_stride = history_stride;
    a.history_len = history_len; a.penalty = penalty; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p;
    a.step = step; a.out_id = out_id; a.out_kept = out_kept;
    if (rows > 1) {
        a.jumps = xorwow_jump_table();
        LLMI_REQUIRE(a.jumps != nullptr, "sample_nucleus: cannot place the XORWOW jump table on the device");
    }
    return nucleus_dispatch(a, rows, s);
}

int engine_nucleus_check(int vocab, float penalty, float temperature, int top_k, float top_p) {
    return nucleus_check_params("set_sampling_params", vocab, penalty, temperature, top_k, top_p);
}

int engine_nucleus_launch(const DecodeState* st, const float* logits, int vocab, const int32_t* tokens, float penalty,
                          float temperature, int top_k, float top_p, uint64_t seed, unsigned long long* partials,
                          int np, hipStream_t s) {
    LLMI_REQUIRE(st && logits && tokens && partials && np >= 1, "engine_nucleus: bad arguments");
    NucArgs a{};
    a.logits = logits; a.vocab = vocab; a.history = tokens; a.penalty = penalty; a.temperature = temperature;
    a.top_k = top_k; a.top_p = top_p; a.step = seed; a.st = st; a.partials = partials; a.np = np;
    return nucleus_dispatch(a, 1, s);
}

}  // namespace llmi
