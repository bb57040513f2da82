// Per-token log-probabilities over a whole logits row (llmi_logprobs,
// llmi_engine_set_logprobs). The reference has no such operator; the rule is this
// project's own (DESIGN.md "Log-probabilities"), restated in numpy by tests/logprob_ref.py:
//   z_i = the RAW logit: no repetition penalty and no temperature. Logprobs describe the
//   model's distribution, not the one a sampler draws from after transforming it.
//   NaN -> -inf; m = max z; order = argmax_key order (value descending, ties to the lower id);
//   w_i = rint((double)expf(z_i - m) * 2^32) as uint64, and an id whose key equals the
//   maximum key has w_i = 2^32 exactly and z_i - m := 0 (weight_of, as nucleus.hip: +inf
//   entries get -log(count), a row of only -inf / NaN gets -log(vocab) everywhere);
//   S = sum w_i over integers: exact in any order;
//   logprob_i = (float)(((double)z_i - (double)m) - log((double)S * 2^-32)), in double;
//   logsumexp = (float)((double)m + log((double)S * 2^-32));
//   top-n = the first n of the order (n rounds of a block maximum over the keys strictly
//   below the previous winner), padded with id -1 / logprob -inf when n > vocab.
//
// One workgroup of 1024 lanes per row, one launch. The row is read once (16-byte loads where
// the row is aligned), turned into 32-bit ordered keys and kept in LDS (vocab <= 32768:
// 128 KB); larger rows (<= 131072) recompute the key from the L2-resident row in every
// pass. Shuffles and LDS only: no global atomics, no cross-workgroup traffic, no allocation.
#include <vector>

#include "kernels.h"
#include "rowkeys.h"

namespace llmi {
namespace {

constexpr int kLpLdsVocab = 32768;   // keys held in LDS up to here
constexpr int kLpMaxVocab = 131072;
constexpr int kLpMaxTop = 8;
constexpr int kLpScratchBytes = 512;

struct LpArgs {
    const float* logits;
    int vocab;
    const int32_t* ids;  // operator form: the scored id per row (null: none)
    int n_top;
    float* out_lp;       // [rows] (operator) / [max_seq + 1] records (engine)
    int32_t* top_ids;    // [rows or records][n_top]
    float* top_lp;
    float* out_lse;      // operator form, nullable
    // engine form: record q = cur_pos + 1, the token step_start will pick for it
    const DecodeState* st;
    const int32_t* prompt;
    const unsigned long long* partials;
    int np;
    int max_seq;
    // row-record form (the scored prefill): rec0 > 0, block b = record rec0 + b, id prompt[rec0 + b]
    int rec0;
};

struct LpScratch {
    unsigned long long red[kRowWaves];
    unsigned long long best[kRowWaves];
    uint32_t mk[kRowWaves];
};

__device__ __forceinline__ uint32_t lp_key(float z) {
    if (z != z) z = -INFINITY;
    return key_of(z);
}

// block maximum of a 64-bit key (0 = none); every lane gets it
__device__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long t = __shfl_xor(v, off, kWave);
        v = t > v ? t : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRowWaves; ++i) v = red[i] > v ? red[i] : v;
    return v;
}

template <bool kLds>
__global__ __launch_bounds__(kRowThreads) void logprob_kernel(LpArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LpScratch* sc = reinterpret_cast<LpScratch*>(smem);
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + kLpScratchBytes);
    const int V = a.vocab;
    const int b = blockIdx.x;
    const float* row = a.logits + (size_t)b * V;
    auto key = [&](int i) -> uint32_t { return kLds ? keys[i] : lp_key(row[i]); };

    // the row, once: keys into LDS, the maximum key
    uint32_t mk = 0u;
    if (kLds) {
        const int head = min(V, (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u));
        const int nv = (V - head) / 4;
        for (int v = threadIdx.x; v < nv; v += kRowThreads) {
            const int i = head + 4 * v;
            const float4 x = *reinterpret_cast<const float4*>(row + i);
            const uint32_t k0 = lp_key(x.x), k1 = lp_key(x.y), k2 = lp_key(x.z), k3 = lp_key(x.w);
            keys[i] = k0; keys[i + 1] = k1; keys[i + 2] = k2; keys[i + 3] = k3;
            mk = max(max(mk, k0), max(k1, max(k2, k3)));
        }
        const int rest = V - 4 * nv;  // head + tail elements, scalar (at most 6)
        if ((int)threadIdx.x < rest) {
            const int i = (int)threadIdx.x < head ? (int)threadIdx.x : 4 * nv + (int)threadIdx.x;
            const uint32_t k = lp_key(row[i]);
            keys[i] = k;
            mk = max(mk, k);
        }
    } else {
        for (int i = threadIdx.x; i < V; i += kRowThreads) mk = max(mk, lp_key(row[i]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mk = max(mk, (uint32_t)__shfl_xor(mk, off, kWave));
    if ((threadIdx.x & 63) == 0) sc->mk[threadIdx.x >> 6] = mk;
    __syncthreads();  // also: every key is in LDS
#pragma unroll
    for (int j = 0; j < kRowWaves; ++j) mk = max(mk, sc->mk[j]);
    const uint32_t mkey = mk;
    const float m = z_of(mkey);

    unsigned long long s = 0;
    for (int i = threadIdx.x; i < V; i += kRowThreads) s += weight_of(key(i), mkey, m);
    const unsigned long long S = block_sum_u64(s, sc->red);  // >= 2^32: the maximum's own weight
    const double lz = log((double)S * (1.0 / 4294967296.0));
    auto lp_of = [&](uint32_t k) -> float {
        return (float)((k == mkey ? 0.0 : (double)z_of(k) - (double)m) - lz);
    };

    // where this row's results go, and the scored id
    int rec = b, tok = -1;
    if (a.st) {
        rec = a.st->cur_pos + 1;
        if (rec < a.st->prompt_len) {
            tok = a.prompt[rec];
        } else {
            unsigned long long best = 0;
            for (int i = threadIdx.x; i < a.np; i += kRowThreads) best = a.partials[i] > best ? a.partials[i] : best;
            tok = (int)argmax_key_index(block_max_u64(best, sc->best));
        }
        if (tok < 0 || tok >= V) tok = 0;  // as step_start_kernel (which also raises the error flag)
        if (rec > a.max_seq) return;       // uniform; the host guards this
    } else if (a.rec0 > 0) {
        rec = a.rec0 + b;
        tok = a.prompt[rec];
        if (tok < 0 || tok >= V) tok = 0;  // as the engine form
    } else if (a.ids) {
        tok = a.ids[b];
    }
    if (threadIdx.x == 0) {
        if (tok >= 0 && tok < V) a.out_lp[rec] = lp_of(key(tok));
        if (a.out_lse) a.out_lse[rec] = (float)((double)m + lz);
    }

    // top-n: the order's first n, one block maximum each
    unsigned long long prev = ~0ull;
    for (int t = 0; t < a.n_top; ++t) {
        unsigned long long best = 0;
        for (int i = threadIdx.x; i < V; i += kRowThreads) {
            const unsigned long long k = ((unsigned long long)key(i) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
            if (k < prev && k > best) best = k;
        }
        best = block_max_u64(best, sc->best);
        if (threadIdx.x == 0) {
            const size_t o = (size_t)rec * a.n_top + t;
            a.top_ids[o] = best ? (int32_t)argmax_key_index(best) : -1;
            a.top_lp[o] = best ? lp_of((uint32_t)(best >> 32)) : -INFINITY;
        }
        prev = best;  // 0 once the row is exhausted: nothing is below it
    }
}

size_t logprob_lds_bytes(int vocab, bool lds) {
    return kLpScratchBytes + (lds ? (((size_t)vocab + 3) & ~(size_t)3) * 4 : 0);
}

int logprob_dispatch(const LpArgs& a, int rows, hipStream_t s) {
    static_assert(sizeof(LpScratch) <= kLpScratchBytes, "scratch region");
    const bool lds = a.vocab <= kLpLdsVocab;
    static const hipError_t attr = [] {  // once: the LDS-resident form's 128.5 KB
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&logprob_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)logprob_lds_bytes(kLpLdsVocab, true));
    }();
    LLMI_HIP(attr);
    const size_t bytes = logprob_lds_bytes(a.vocab, lds);
    if (lds)
        hipLaunchKernelGGL(logprob_kernel<true>, dim3(rows), dim3(kRowThreads), bytes, s, a);
    else
        hipLaunchKernelGGL(logprob_kernel<false>, dim3(rows), dim3(kRowThreads), bytes, s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int logprob_check(const char* who, int vocab, int n_top) {
    const std::string w(who);
    LLMI_REQUIRE(vocab > 0, w + ": vocab must be positive");
    LLMI_REQUIRE(n_top >= 0 && n_top <= kLpMaxTop, w + ": n_top must be in [0, 8]");
    if (vocab > kLpMaxVocab) {
        set_last_error("[llmi][ERROR] " + w + ": vocab above 131072 is not supported");
        return LLMI_EUNSUPPORTED;
    }
    return LLMI_OK;
}

}  // namespace

int logprobs_launch(const float* logits, int rows, int vocab, const int32_t* ids, int n_top, float* out_lp,
                    int32_t* top_ids, float* top_lp, float* out_lse, hipStream_t s) {
    LLMI_REQUIRE(logits, "logprobs: null logits");
    LLMI_REQUIRE(rows > 0 && rows <= 65536, "logprobs: rows must be in [1, 65536]");
    LLMI_TRY(logprob_check("logprobs", vocab, n_top));
    LLMI_REQUIRE(!ids || out_lp, "logprobs: ids without out_lp");
    LLMI_REQUIRE(n_top == 0 || (top_ids && top_lp), "logprobs: n_top > 0 needs top_ids and top_lp");
    if (ids) {
        // ids are checked on the host unless the stream is capturing (no copies inside a
        // capture); the kernel itself writes nothing for an id outside [0, vocab)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        LLMI_HIP(hipStreamIsCapturing(s, &cap));
        if (cap == hipStreamCaptureStatusNone) {
            std::vector<int32_t> h(rows);
            LLMI_HIP(hipMemcpyAsync(h.data(), ids, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
            LLMI_HIP(hipStreamSynchronize(s));
            for (int32_t id : h) LLMI_REQUIRE(id >= 0 && id < vocab, "logprobs: ids must be in [0, vocab)");
        }
    }
    LpArgs a{};
    a.logits = logits; a.vocab = vocab; a.ids = ids; a.n_top = n_top; a.out_lp = out_lp; a.top_ids = top_ids;
    a.top_lp = top_lp; a.out_lse = out_lse;
    return logprob_dispatch(a, rows, s);
}

int engine_logprob_check(int vocab, int n_top) { return logprob_check("set_logprobs", vocab, n_top); }

int engine_logprob_launch(const DecodeState* st, const float* logits, int vocab, const int32_t* prompt,
                          const unsigned long long* partials, int np, int max_seq, int n_top, float* tok_lp,
                          int32_t* top_ids, float* top_lp, hipStream_t s) {
    LLMI_REQUIRE(st && logits && prompt && partials && np >= 1 && tok_lp, "engine_logprob: bad arguments");
    LLMI_REQUIRE(n_top == 0 || (top_ids && top_lp), "engine_logprob: n_top > 0 needs top_ids and top_lp");
    LpArgs a{};
    a.logits = logits; a.vocab = vocab; a.n_top = n_top; a.out_lp = tok_lp; a.top_ids = top_ids; a.top_lp = top_lp;
    a.st = st; a.prompt = prompt; a.partials = partials; a.np = np; a.max_seq = max_seq;
    return logprob_dispatch(a, 1, s);
}

int engine_logprob_rows_launch(const float* slab, int rows, int vocab, const int32_t* prompt, int rec0, int max_seq,
                               int n_top, float* tok_lp, int32_t* top_ids, float* top_lp, hipStream_t s) {
    LLMI_REQUIRE(slab && prompt && tok_lp && rows >= 1, "engine_logprob_rows: bad arguments");
    LLMI_REQUIRE(rec0 >= 1 && rec0 + rows <= max_seq, "engine_logprob_rows: records must lie inside the prompt");
    LLMI_REQUIRE(n_top == 0 || (top_ids && top_lp), "engine_logprob_rows: n_top > 0 needs top_ids and top_lp");
    LpArgs a{};
    a.logits = slab; a.vocab = vocab; a.n_top = n_top; a.out_lp = tok_lp; a.top_ids = top_ids; a.top_lp = top_lp;
    a.prompt = prompt; a.rec0 = rec0; a.max_seq = max_seq;
    return logprob_dispatch(a, rows, s);
}

}  // namespace llmi
