// Forking a sequence (engine.h; include/llmi.h has the contract of llmi_batch_fork): copy one
// engine's sequence into up to 7 others on the same stream -- a batch's slots -- so that several
// continuations of one prompt cost one prompt pass. Two stream-ordered launches: the cache rows
// [0, keep) of every layer (kv_fork.hip: each source byte read once, stored once per
// destination) and the small per-sequence state below. The cut form leaves every destination
// where edit(keep, ids, n) would leave the source; the continue form (n == 0) leaves it where the
// source stands, pending token included. Like edit it clears nothing and moves no buffer: rows
// and ids at or after `keep` are stale in a destination and are rewritten by the step that
// reaches them before anything reads them, and the captured step graphs stay valid.
#include "engine.h"

namespace llmi {
namespace {

constexpr int kForkT = 256;
constexpr int kForkByValue = 8;  // ids that travel in the launch arguments (as edit's)

struct ForkSeq {  // one sequence's buffers, as 32-bit words where they are only copied
    DecodeState* st;
    int32_t* prompt;
    int32_t* tokens;
    unsigned* partials;  // [np u64]
    unsigned* logits;    // [vocab]
    unsigned* lr_out;    // [vocab]; null unless source and destination both have rules on
    unsigned* lp;        // the logprob blob; null: the destination has none
    int lp_copy;         // source and destination record with the same n_top
};
struct ForkArgs {
    ForkSeq src;
    ForkSeq dst[kKvCopyMaxDst];
    int cont;        // the continue form
    int keep, n;
    int n_val;       // by-value ids (0: a longer list was copied before the launch)
    int32_t ids[kForkByValue];
    int src_plen;    // continue form: the source's prompt length
    int vocab, np;
    int records;     // logprob records of an engine (max_seq + 1)
    int lp_stride;   // the source's record stride of the two top arrays
};

template <typename T>
__device__ __forceinline__ void copy_words(T* d, const T* s, size_t n, size_t t, size_t step) {
    for (size_t i = t; i < n; i += step) d[i] = s[i];
}

// blockIdx.y: the destination. Its decode state (epoch stays: the fused q/k/v launch's granule
// tags must never repeat), ids, prompt and -- continue form -- pending token and logits rows; its
// logprob records: the source's below the cut where lp_copy, every other one "not computed"
// (every byte 0xFF: NaN / id -1; the blob is tok_lp [records], top_ids and top_lp
// [records * 8] each).
__global__ __launch_bounds__(kForkT) void seq_fork_kernel(ForkArgs a) {
    const ForkSeq& D = a.dst[blockIdx.y];
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (t == 0) {
        D.st->next_pos = a.cont ? a.src.st->next_pos : a.keep;
        D.st->cur_pos = a.cont ? a.src.st->cur_pos : (a.keep > 0 ? a.keep - 1 : 0);
        D.st->prompt_len = a.cont ? a.src.st->prompt_len : a.keep + a.n;
        D.st->vocab = a.vocab;
        D.st->error = a.src.st->error;
    }
    copy_words(D.tokens, a.src.tokens, (size_t)a.keep, t, step);
    if (a.cont) {
        copy_words(D.prompt, a.src.prompt, (size_t)a.src_plen, t, step);
        copy_words(D.partials, a.src.partials, (size_t)a.np * 2, t, step);
        copy_words(D.logits, a.src.logits, (size_t)a.vocab, t, step);
        if (D.lr_out) copy_words(D.lr_out, a.src.lr_out, (size_t)a.vocab, t, step);
    } else {
        copy_words(D.prompt, a.src.tokens, (size_t)a.keep, t, step);
        if (t < (size_t)a.n_val) D.prompt[a.keep + t] = a.ids[t];
    }
    if (!D.lp) return;
    const size_t R = (size_t)a.records, top = R * Engine::kLpMaxTop;
    const size_t nrec = D.lp_copy ? (size_t)a.keep + (a.cont ? 1 : 0) : 0;
    const size_t nw = nrec * (size_t)(a.lp_stride > 0 ? a.lp_stride : 0);
    for (size_t q = t; q < R; q += step) D.lp[q] = q < nrec ? a.src.lp[q] : 0xFFFFFFFFu;
    for (size_t i = t; i < top; i += step) {
        D.lp[R + i] = i < nw ? a.src.lp[R + i] : 0xFFFFFFFFu;
        D.lp[R + top + i] = i < nw ? a.src.lp[R + top + i] : 0xFFFFFFFFu;
    }
}

}  // namespace

// `dst`: other engines on this engine's stream with this engine's configuration (a batch's slots)
int Engine::fork_into(const std::vector<Engine*>& dst, int keep, const int32_t* ids, int n) {
    if (decode_mode == 1) {
        set_last_error("[llmi][ERROR] fork: the ring decode mode keeps a sequence it cannot copy (set_decode_mode 0)");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_REQUIRE(prompt_len > 0, "fork: the source is idle (set_prompt first)");
    LLMI_REQUIRE(!dst.empty() && (int)dst.size() <= kKvCopyMaxDst, "fork: 1..7 destinations");
    for (size_t i = 0; i < dst.size(); ++i) {
        LLMI_REQUIRE(dst[i] && dst[i] != this, "fork: a destination is the source");
        for (size_t j = 0; j < i; ++j) LLMI_REQUIRE(dst[i] != dst[j], "fork: a destination is listed twice");
        LLMI_REQUIRE(dst[i]->stream == stream && dst[i]->c.max_seq == c.max_seq && dst[i]->c.vocab == c.vocab &&
                         dst[i]->c.layers == c.layers && dst[i]->kvl == kvl && dst[i]->c.head_dim == c.head_dim &&
                         dst[i]->c.kv_dtype == c.kv_dtype && dst[i]->lm_grid == lm_grid && dst[i]->decode_mode != 1,
                     "fork: source and destination must share a stream and a configuration");
    }
    LLMI_REQUIRE(keep >= 0 && keep <= host_next_pos, "fork: keep must be in [0, next position]");
    LLMI_REQUIRE(n >= 0 && n <= c.max_seq - keep, "fork: need n >= 0 and keep + n <= max_seq");
    LLMI_REQUIRE(n == 0 || ids != nullptr, "fork: null ids");
    for (int i = 0; i < n; ++i) LLMI_REQUIRE(ids[i] >= 0 && ids[i] < c.vocab, "fork: token id out of range");
    LLMI_REQUIRE(n >= 1 || keep == host_next_pos,
                 "fork: a cut needs at least one forced id (the pending token is forgotten)");
    const bool cont = n == 0;

    KvCopyArgs kv;
    kv.src_k = kcache; kv.src_v = vcache; kv.src_k_scale = kscale; kv.src_v_scale = vscale;
    for (size_t i = 0; i < dst.size(); ++i) {
        kv.dst_k[i] = dst[i]->kcache; kv.dst_v[i] = dst[i]->vcache;
        kv.dst_k_scale[i] = dst[i]->kscale; kv.dst_v_scale[i] = dst[i]->vscale;
    }
    kv.n_dst = (int)dst.size();
    kv.cache_dtype = c.kv_dtype;
    kv.layers = c.layers; kv.kv_heads = kvl; kv.max_seq = c.max_seq; kv.head_dim = c.head_dim;
    kv.n_rows = keep;
    kv.n_cu = n_cu;
    LLMI_TRY(kv_copy_rows_launch(kv, stream));  // (refuses before it launches: nothing has changed)

    auto seq_of = [](const Engine& e) {
        ForkSeq s{};
        s.st = e.st; s.prompt = e.prompt; s.tokens = e.tokens;
        s.partials = reinterpret_cast<unsigned*>(e.partials);
        s.logits = reinterpret_cast<unsigned*>(e.logits);
        s.lp = reinterpret_cast<unsigned*>(e.lp_buf);
        return s;
    };
    ForkArgs a{};
    a.src = seq_of(*this);
    a.src.lr_out = reinterpret_cast<unsigned*>(rules_on() ? lr_out : nullptr);
    for (size_t i = 0; i < dst.size(); ++i) {
        const Engine& d = *dst[i];
        a.dst[i] = seq_of(d);
        a.dst[i].lr_out = reinterpret_cast<unsigned*>(a.src.lr_out && d.rules_on() ? d.lr_out : nullptr);
        a.dst[i].lp_copy = lp_buf && d.lp_buf && lp_top >= 0 && d.lp_top == lp_top;
    }
    a.cont = cont;
    a.keep = keep;
    a.n = n;
    a.n_val = n <= kForkByValue ? n : 0;
    for (int i = 0; i < a.n_val; ++i) a.ids[i] = ids[i];
    a.src_plen = prompt_len;
    a.vocab = c.vocab;
    a.np = lm_grid;
    a.records = (int)lp_records();
    a.lp_stride = lp_stride;
    for (Engine* d : dst)
        if (n > kForkByValue)
            LLMI_HIP(hipMemcpyAsync(d->prompt + keep, ids, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    const size_t work = std::max<size_t>((size_t)c.vocab, lp_records() * kLpMaxTop);
    const int grid = (int)std::min<size_t>(64, (work + kForkT - 1) / kForkT);
    hipLaunchKernelGGL(seq_fork_kernel, dim3(std::max(grid, 1), (unsigned)dst.size()), dim3(kForkT), 0, stream, a);
    LLMI_HIP(hipGetLastError());
    if (n > kForkByValue) LLMI_HIP(hipStreamSynchronize(stream));  // the caller's ids were read from pageable memory
    for (Engine* d : dst) {
        d->host_next_pos = keep;
        d->prompt_len = cont ? prompt_len : keep + n;
        d->sc_m = 0;  // the logits slab holds no row of this sequence
    }
    return LLMI_OK;
}

// slot src into the slots dst[0 .. n_dst); keep -1: the source's position
int Batch::fork(int src, const int* dst, int n_dst, int keep, const int32_t* ids, int n) {
    LLMI_TRY(slot_ok(src));
    LLMI_REQUIRE(n_dst >= 1 && n_dst <= kKvCopyMaxDst && dst, "batch fork: 1..7 destinations");
    std::vector<Engine*> to;
    for (int i = 0; i < n_dst; ++i) {
        LLMI_REQUIRE(dst[i] >= 0 && dst[i] < (int)r.size(), "batch fork: a destination is out of range");
        LLMI_REQUIRE(dst[i] != src, "batch fork: a destination is the source");
        for (int j = 0; j < i; ++j) LLMI_REQUIRE(dst[i] != dst[j], "batch fork: a destination is listed twice");
        to.push_back(r[dst[i]].get());
    }
    LLMI_REQUIRE(r[src]->prompt_len > 0, "batch fork: the source slot is idle (set_prompt first)");
    return r[src]->fork_into(to, keep == -1 ? r[src]->host_next_pos : keep, ids, n);
}

}  // namespace llmi
