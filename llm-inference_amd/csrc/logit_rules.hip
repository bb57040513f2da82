// Logit rules over whole logits rows (llmi_process_logits):
// additive bias (a -inf bias bans an id), presence / frequency penalties over a history of
// ids, and an allowed-token bitmap. The reference has no such operator; the rule is this
// project's own (DESIGN.md "Logit rules"), restated in numpy by tests/logit_rules_ref.py.
// For id i of the raw row z, in this order, every step ONE round-to-nearest fp32 operation
// (mul_rn / add_rn / sub_rn below: never contracted into an fma):
//   1. v = z[i]; NaN -> -inf (the nucleus sampler's convention);
//   2. bias b (nullable): if b[i] != 0, v = v + b[i]    (-0.0 + 0.0 would give +0.0, which
//      argmax_key orders above -0.0: a zero bias must leave the bits alone);
//   3. c = occurrences of i in the history; if c > 0 and a penalty is non-zero:
//      t = frequency * (float)c; t = presence + t; v = v - t;
//      a NaN that steps 2 and 3 produce (+inf meeting -inf) -> -inf, as in step 1;
//   4. allowed bitmap (nullable): bit i & 31 of word i >> 5 clear -> v = -inf.
// Outputs: the processed row (a second buffer: the raw row is never written) and the id of
// max_i argmax_key(v[i], i) -- value descending, ties to the lower id, an all -inf row id 0.
//
// One workgroup of 1024 lanes per row, one launch. The row is read once (16-byte loads
// where the row is aligned) and the processed row written once. The counts are 16-bit LDS
// counters, two per u32 word, filled with LDS integer atomics (exact in any order): 65536
// ids take 128 KB, so a row above 65536 ids runs two passes over its id halves and scans
// the history once per pass; a history holds at most 65535 ids, so no counter overflows
// into its neighbour. With both penalties zero nothing is counted and no LDS but the
// reduction's is claimed. No global atomics, no cross-workgroup traffic, no allocation.
//
// Two kernels share the per-id arithmetic (lr_apply), the counter fill and the key reduction:
// the operator's (any alignment, rows of a batch, histories given as arrays) and the engine
// form (engine_logit_rules_launch: one row, the history read from the device decode state,
// 16-byte loads of row, bias and output, the winner left as an argmax partial).
#include <algorithm>
#include <cmath>
#include <vector>

#include "kernels.h"
#include "rowkeys.h"

// HIP's __fmul_rn / __fadd_rn / __fsub_rn are inline functions around the plain operators,
// compiled under the default -ffp-contract=fast: once inlined, frequency * c + presence
// becomes one v_fma_f32 (one rounding, not the rule's two). The three operations are
// therefore written here, under a pragma that keeps the contract flag off them.
#pragma clang fp contract(off)

namespace llmi {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kLrMaxVocab = 131072;
constexpr int kLrHalf = 65536;       // ids per counting pass
constexpr int kLrMaxHistory = 65535;  // a 16-bit counter's range
constexpr int kLrScratchBytes = 512;

struct LrArgs {
    const float* logits;
    int vocab;
    const float* bias;        // [vocab], nullable, shared by the rows
    const uint32_t* allowed;  // nullable
    int allowed_stride;       // words per row; 0: one bitmap for all rows
    const int32_t* history;
    int history_stride;
    const int32_t* history_len;  // null: no history
    float presence, frequency;
    float* out;
    int32_t* out_ids;
};

struct LrScratch {
    unsigned long long best[kRowWaves];
};

// Steps 1-4 for one id, shared by the operator and the engine form: bi the id's bias (0: none),
// c its count in the history (0: none, or no penalty is set), ok its bit of the allowed bitmap.
__device__ __forceinline__ float lr_apply(float v, float bi, uint32_t c, float presence, float frequency, bool ok) {
    if (v != v) v = -INFINITY;
    if (bi != 0.f) v = add_rn(v, bi);
    if (c) {
        float t = mul_rn(frequency, (float)c);
        t = add_rn(presence, t);
        v = sub_rn(v, t);
    }
    if (v != v) v = -INFINITY;
    if (!ok) v = -INFINITY;
    return v;
}
// the 16-bit counter of id lo + j (cnt holds ids [lo, lo + kLrHalf))
__device__ __forceinline__ uint32_t lr_count(const uint32_t* cnt, int j) {
    return (cnt[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
}
// The counters of ids [lo, hi) over hist[0 .. n_hist), by the whole workgroup; resync: an
// earlier pass may still be reading cnt. Ids outside [lo, hi) are skipped.
__device__ __forceinline__ void lr_fill_counts(uint32_t* cnt, const int32_t* hist, int n_hist, int lo, int hi,
                                               bool resync) {
    const int words = (hi - lo + 1) / 2;
    if (resync) __syncthreads();
    for (int w = threadIdx.x; w < words; w += kRowThreads) cnt[w] = 0u;
    __syncthreads();
    for (int h = threadIdx.x; h < n_hist; h += kRowThreads) {
        const int id = hist[h];
        if (id >= lo && id < hi) atomicAdd(&cnt[(id - lo) >> 1], 1u << (((id - lo) & 1) * 16));
    }
    __syncthreads();
}
// the workgroup's maximum key, in every lane (every key is non-zero: v is never NaN)
__device__ __forceinline__ unsigned long long lr_block_best(unsigned long long best, LrScratch* sc) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long t = __shfl_xor(best, off, kWave);
        best = t > best ? t : best;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc->best[threadIdx.x >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRowWaves; ++i) best = sc->best[i] > best ? sc->best[i] : best;
    return best;
}

__global__ __launch_bounds__(kRowThreads) void logit_rules_kernel(LrArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LrScratch* sc = reinterpret_cast<LrScratch*>(smem);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + kLrScratchBytes);
    const int V = a.vocab;
    const int b = blockIdx.x;
    const float* row = a.logits + (size_t)b * V;
    float* out = a.out + (size_t)b * V;
    const uint32_t* allowed = a.allowed ? a.allowed + (size_t)b * a.allowed_stride : nullptr;

    const int32_t* hist = a.history;
    int n_hist = 0;
    if (a.history_len) {
        n_hist = min(max(a.history_len[b], 0), a.history_stride);
        hist += (size_t)b * a.history_stride;
    }
    n_hist = min(n_hist, kLrMaxHistory);  // (the host refuses longer histories)
    const bool pen = (a.presence != 0.f || a.frequency != 0.f) && n_hist > 0;
    const float presence = a.presence, frequency = a.frequency;
    const float* bias = a.bias;

    unsigned long long best = 0ull;
    // ids [lo, hi), counters of ids [lo, lo + kLrHalf) in cnt when pen
    auto one = [&](float v, int i, int lo) -> float {
        v = lr_apply(v, bias ? bias[i] : 0.f, pen ? lr_count(cnt, i - lo) : 0u, presence, frequency,
                     !allowed || ((allowed[i >> 5] >> (i & 31)) & 1u));
        const unsigned long long k = argmax_key(v, (uint32_t)i);
        best = k > best ? k : best;
        return v;
    };

    const int passes = pen ? (V + kLrHalf - 1) / kLrHalf : 1;
    for (int p = 0; p < passes; ++p) {
        const int lo = pen ? p * kLrHalf : 0;
        const int hi = pen ? min(V, lo + kLrHalf) : V;
        if (pen) lr_fill_counts(cnt, hist, n_hist, lo, hi, p > 0);
        const float* src = row + lo;
        float* dst = out + lo;
        const int n = hi - lo;
        const int head = min(n, (int)((4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u));
        const int nv = (n - head) / 4;
        const bool vst = (((uintptr_t)(dst + head)) & 15u) == 0;
        for (int q = threadIdx.x; q < nv; q += kRowThreads) {
            const int j = head + 4 * q, i = lo + j;
            const float4 x = *reinterpret_cast<const float4*>(src + j);
            float4 y;
            y.x = one(x.x, i, lo); y.y = one(x.y, i + 1, lo); y.z = one(x.z, i + 2, lo); y.w = one(x.w, i + 3, lo);
            if (vst) {
                *reinterpret_cast<float4*>(dst + j) = y;
            } else {
                dst[j] = y.x; dst[j + 1] = y.y; dst[j + 2] = y.z; dst[j + 3] = y.w;
            }
        }
        const int rest = n - 4 * nv;  // head + tail elements, scalar (at most 6)
        if ((int)threadIdx.x < rest) {
            const int j = (int)threadIdx.x < head ? (int)threadIdx.x : 4 * nv + (int)threadIdx.x;
            dst[j] = one(src[j], lo + j, lo);
        }
    }

    best = lr_block_best(best, sc);
    if (threadIdx.x == 0) a.out_ids[b] = (int32_t)argmax_key_index(best);
}

// The engine form (engine_logit_rules_launch): one row, the history tokens[h0 .. cur_pos] of
// the device decode state (h0 = 0 when the prompt counts, else prompt_len; on a prompt step the
// window is empty), the winner left as the only non-zero argmax partial (sample_pick_kernel's
// convention). The row, the bias and out are 16-byte aligned engine buffers and the counting
// passes start at multiples of 65536 ids, so all three move as float4 and the four ids of a
// vector share one word of the bitmap (always present: all ones = no mask).
struct LrEngArgs {
    const DecodeState* st;
    const float* logits;
    int vocab;
    const float* bias;        // [vocab], nullable
    const uint32_t* allowed;  // [(vocab + 31) / 32]
    const int32_t* tokens;
    int count_prompt;
    float presence, frequency;
    float* out;
    unsigned long long* partials;
    int np;
};

__global__ __launch_bounds__(kRowThreads) void engine_logit_rules_kernel(LrEngArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LrScratch* sc = reinterpret_cast<LrScratch*>(smem);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + kLrScratchBytes);
    const int V = a.vocab;
    const int h0 = a.count_prompt ? 0 : a.st->prompt_len;
    const int n_hist = min(max(a.st->cur_pos + 1 - h0, 0), kLrMaxHistory);
    const int32_t* hist = a.tokens + h0;
    const bool pen = (a.presence != 0.f || a.frequency != 0.f) && n_hist > 0;
    const float presence = a.presence, frequency = a.frequency;
    const float* bias = a.bias;
    const uint32_t* allowed = a.allowed;

    unsigned long long best = 0ull;
    auto keep = [&](float v, int i) {
        const unsigned long long k = argmax_key(v, (uint32_t)i);
        best = k > best ? k : best;
    };
    const int passes = pen ? (V + kLrHalf - 1) / kLrHalf : 1;
    for (int p = 0; p < passes; ++p) {
        const int lo = pen ? p * kLrHalf : 0;
        const int hi = pen ? min(V, lo + kLrHalf) : V;
        if (pen) lr_fill_counts(cnt, hist, n_hist, lo, hi, p > 0);
        const int n = hi - lo, nv = n / 4;
        const float4* src = reinterpret_cast<const float4*>(a.logits + lo);
        const float4* bsrc = bias ? reinterpret_cast<const float4*>(bias + lo) : nullptr;
        float4* dst = reinterpret_cast<float4*>(a.out + lo);
        for (int q = threadIdx.x; q < nv; q += kRowThreads) {
            const int j = 4 * q, i = lo + j;  // i % 4 == 0: bits i .. i + 3 of one bitmap word
            const float4 x = src[q];
            const float4 bi = bsrc ? bsrc[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t ok = allowed[i >> 5] >> (i & 31);
            uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
            if (pen) {
                const uint32_t w0 = cnt[2 * q], w1 = cnt[2 * q + 1];
                c0 = w0 & 0xFFFFu; c1 = w0 >> 16; c2 = w1 & 0xFFFFu; c3 = w1 >> 16;
            }
            float4 y;
            y.x = lr_apply(x.x, bi.x, c0, presence, frequency, ok & 1u);
            y.y = lr_apply(x.y, bi.y, c1, presence, frequency, (ok >> 1) & 1u);
            y.z = lr_apply(x.z, bi.z, c2, presence, frequency, (ok >> 2) & 1u);
            y.w = lr_apply(x.w, bi.w, c3, presence, frequency, (ok >> 3) & 1u);
            keep(y.x, i); keep(y.y, i + 1); keep(y.z, i + 2); keep(y.w, i + 3);
            dst[q] = y;
        }
        const int j = 4 * nv + (int)threadIdx.x;  // the tail: at most 3 ids
        if (j < n) {
            const int i = lo + j;
            const float v = lr_apply(a.logits[i], bias ? bias[i] : 0.f, pen ? lr_count(cnt, j) : 0u, presence,
                                     frequency, (allowed[i >> 5] >> (i & 31)) & 1u);
            keep(v, i);
            a.out[i] = v;
        }
    }

    best = lr_block_best(best, sc);
    if (threadIdx.x == 0) a.partials[0] = argmax_key(1.0f, argmax_key_index(best));
    for (int i = 1 + threadIdx.x; i < a.np; i += kRowThreads) a.partials[i] = 0ull;
}

size_t logit_rules_lds_bytes(int vocab, bool pen) {
    return kLrScratchBytes + (pen ? (size_t)((std::min(vocab, kLrHalf) + 1) / 2) * 4 : 0);
}

int logit_rules_dispatch(const LrArgs& a, int rows, hipStream_t s) {
    static_assert(sizeof(LrScratch) <= kLrScratchBytes, "scratch region");
    static const hipError_t attr = [] {  // once: the counters' 128 KB
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&logit_rules_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)logit_rules_lds_bytes(kLrHalf, true));
    }();
    LLMI_HIP(attr);
    const bool pen = (a.presence != 0.f || a.frequency != 0.f) && a.history_len;
    hipLaunchKernelGGL(logit_rules_kernel, dim3(rows), dim3(kRowThreads), logit_rules_lds_bytes(a.vocab, pen), s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int logit_rules_check(const char* who, int vocab, float presence, float frequency) {
    const std::string w(who);
    LLMI_REQUIRE(vocab > 0, w + ": vocab must be positive");
    LLMI_REQUIRE(std::isfinite(presence) && std::isfinite(frequency), w + ": the penalties must be finite");
    if (vocab > kLrMaxVocab) {
        set_last_error("[llmi][ERROR] " + w + ": vocab above 131072 is not supported");
        return LLMI_EUNSUPPORTED;
    }
    return LLMI_OK;
}

}  // namespace

int logit_rules_launch(const float* logits, int rows, int vocab, const float* bias, const uint32_t* allowed,
                       int allowed_stride, const int32_t* history, int history_stride, const int32_t* history_len,
                       float presence, float frequency, float* out, int32_t* out_ids, hipStream_t s) {
    LLMI_REQUIRE(logits && out && out_ids, "process_logits: null logits, out or out_ids");
    LLMI_REQUIRE(logits != out, "process_logits: out must not be the logits (the raw row is never written)");
    LLMI_REQUIRE(rows > 0 && rows <= 65536, "process_logits: rows must be in [1, 65536]");
    LLMI_TRY(logit_rules_check("process_logits", vocab, presence, frequency));
    LLMI_REQUIRE(allowed_stride == 0 || (allowed && allowed_stride >= (vocab + 31) / 32),
                 "process_logits: allowed_stride must be 0 (one bitmap) or >= (vocab + 31) / 32 words");
    LLMI_REQUIRE(!history_len || (history && history_stride >= 0),
                 "process_logits: history_len without a history (null pointer or negative stride)");
    if (history_len && history_stride > kLrMaxHistory) {
        set_last_error("[llmi][ERROR] process_logits: a history holds at most 65535 ids (16-bit counters)");
        return LLMI_EUNSUPPORTED;
    }
    // the host checks below read device memory back, so they are skipped while the stream is
    // capturing (no copies inside a capture); the kernel clamps the lengths and skips any id
    // outside [0, vocab)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    LLMI_HIP(hipStreamIsCapturing(s, &cap));
    if (cap == hipStreamCaptureStatusNone) {
        if (bias) {
            std::vector<float> h(vocab);
            LLMI_HIP(hipMemcpyAsync(h.data(), bias, (size_t)vocab * 4, hipMemcpyDeviceToHost, s));
            LLMI_HIP(hipStreamSynchronize(s));
            for (float v : h)
                LLMI_REQUIRE(std::isfinite(v) || (std::isinf(v) && v < 0.f),
                             "process_logits: bias values must be finite or -inf (a ban)");
        }
        if (history_len) {
            std::vector<int32_t> len(rows), ids;
            LLMI_HIP(hipMemcpyAsync(len.data(), history_len, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
            LLMI_HIP(hipStreamSynchronize(s));
            for (int b = 0; b < rows; ++b) {
                LLMI_REQUIRE(len[b] >= 0 && len[b] <= history_stride,
                             "process_logits: history_len must be in [0, history_stride]");
                if (len[b] == 0) continue;
                ids.resize(len[b]);
                LLMI_HIP(hipMemcpyAsync(ids.data(), history + (size_t)b * history_stride, (size_t)len[b] * 4,
                                        hipMemcpyDeviceToHost, s));
                LLMI_HIP(hipStreamSynchronize(s));
                for (int32_t id : ids)
                    LLMI_REQUIRE(id >= 0 && id < vocab, "process_logits: history ids must be in [0, vocab)");
            }
        }
    }
    LrArgs a{};
    a.logits = logits; a.vocab = vocab; a.bias = bias; a.allowed = allowed; a.allowed_stride = allowed_stride;
    a.history = history; a.history_stride = history_stride; a.history_len = history_len;
    a.presence = presence; a.frequency = frequency; a.out = out; a.out_ids = out_ids;
    return logit_rules_dispatch(a, rows, s);
}

int engine_logit_rules_check(int vocab, int max_seq, float presence, float frequency) {
    LLMI_TRY(logit_rules_check("set_logit_rules", vocab, presence, frequency));
    if ((presence != 0.f || frequency != 0.f) && max_seq > kLrMaxHistory) {
        set_last_error("[llmi][ERROR] set_logit_rules: penalties need max_seq <= 65535 (16-bit counters)");
        return LLMI_EUNSUPPORTED;
    }
    return LLMI_OK;
}

// No host read-back and no copy: capturable. The ids of tokens[] are step_start's / prefill_finish's
// own (all in [0, vocab)); the kernel skips any other.
int engine_logit_rules_launch(const DecodeState* st, const float* logits, int vocab, const float* bias,
                              const uint32_t* allowed, const int32_t* tokens, int count_prompt, float presence,
                              float frequency, float* out, unsigned long long* partials, int np, hipStream_t s) {
    LLMI_REQUIRE(st && logits && allowed && tokens && out && partials && np >= 1, "engine_logit_rules: bad arguments");
    LLMI_REQUIRE(logits != out, "engine_logit_rules: out must not be the logits (the raw row is never written)");
    LLMI_REQUIRE(vocab > 0 && vocab <= kLrMaxVocab, "engine_logit_rules: vocab must be in [1, 131072]");
    LLMI_REQUIRE((((uintptr_t)logits | (uintptr_t)out | (uintptr_t)bias) & 15u) == 0,
                 "engine_logit_rules: the row, the bias and out must be 16-byte aligned");
    static const hipError_t attr = [] {  // once: the counters' 128 KB
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&engine_logit_rules_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)logit_rules_lds_bytes(kLrHalf, true));
    }();
    LLMI_HIP(attr);
    LrEngArgs a{};
    a.st = st; a.logits = logits; a.vocab = vocab; a.bias = bias; a.allowed = allowed; a.tokens = tokens;
    a.count_prompt = count_prompt; a.presence = presence; a.frequency = frequency; a.out = out;
    a.partials = partials; a.np = np;
    const bool pen = presence != 0.f || frequency != 0.f;
    hipLaunchKernelGGL(engine_logit_rules_kernel, dim3(1), dim3(kRowThreads), logit_rules_lds_bytes(vocab, pen), s, a);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace llmi
