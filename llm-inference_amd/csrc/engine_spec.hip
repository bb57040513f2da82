// Speculative decoding on the single-rank engine: the verify step, prompt-lookup drafting and
// the lookup generation loop (engine.h; include/llmi.h has the contract).
//
// A verify step runs the pending token (lane 0: the engine's own buffers) and n_draft proposed
// continuations (lanes 1..n_draft: an Engine each that borrows the weights, the KV cache and
// the RoPE table) through the model as m = n_draft + 1 rows of ONE sequence at positions
// p .. p + m - 1:
//   spec_start (every lane's token + embedding)
//   L x [ gemv_rows q/k/v | attn_rows | oproj_rows | gemv_rows gate_up | gemv_rows down ]
//   gemv_rows lm_head + argmax partials
//   spec_commit (accept on the device, leave the engine where a + 1 plain steps would)
// = 5L + 3 launches that stream every weight and every cached K / V row once. Every multi-row
// launch gives row i bitwise its single-row result (gemv_rows.hip, attn_rows.hip) and the
// residual stream is integer fixed point, so row i's logits are bitwise those of the plain
// step at position p + i after the same tokens: what is accepted is exactly greedy decode.
//
// Proposals come from a host lookup in the sequence itself (generate_lookup) or from a second,
// smaller engine that runs plain token steps and is re-aligned after every verify step with
// Engine::edit (generate_draft); the target's result does not depend on what is proposed.
#include "engine.h"

namespace llmi {
namespace {

constexpr int kSpecT = 1024;

struct SpecLanes {  // per lane: what spec_start writes and spec_commit reads
    int m = 0;
    float* x[kAttnRowsMax];
    long long* res0[kAttnRowsMax];
    long long* xacc[kAttnRowsMax];  // null: the attention launch seeds it
    unsigned long long* partials[kAttnRowsMax];
    float* logits[kAttnRowsMax];
    DecodeState* st[kAttnRowsMax];
};

// the largest key of the block (every thread gets it); sh: kSpecT / 64 words
__device__ unsigned long long spec_block_max(unsigned long long k, unsigned long long* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(k, o, 64);
        k = t > k ? t : k;
    }
    __syncthreads();
    if (lane == 0) sh[w] = k;
    __syncthreads();
    unsigned long long b = sh[0];
    for (int i = 1; i < nw; ++i) b = sh[i] > b ? sh[i] : b;
    return b;
}
__device__ int spec_argmax(const unsigned long long* partials, int np, unsigned long long* sh) {
    unsigned long long best = 0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) best = partials[i] > best ? partials[i] : best;
    return (int)argmax_key_index(spec_block_max(best, sh));
}

// Workgroup i = lane i. Lane 0 is step_start_kernel (ops.hip) on the engine's state: the token
// of position next_pos (the prompt's, or the argmax of the last forward's partials), recorded,
// the position and the epoch advanced. Lane i > 0 takes draft[i - 1]; its token is recorded by
// spec_commit if it is accepted. Every lane gathers its embedding row into x, fixed(x) into
// res[0] and (xacc given) into the o_proj accumulator.
template <typename TT>
__global__ __launch_bounds__(kSpecT) void spec_start_kernel(SpecLanes L, const int32_t* prompt, int np,
                                                            int32_t* tokens, const int32_t* draft, const TT* table,
                                                            int hidden, int max_seq) {
    __shared__ unsigned long long sh[kSpecT / 64];
    __shared__ int tok_s;
    const int lane = blockIdx.x;
    DecodeState* st = L.st[0];
    int tok;
    if (lane == 0) {
        const int p = st->next_pos;
        if (p >= max_seq) {  // host guards this; keep the state consistent if it does not
            if (threadIdx.x == 0) {
                atomicOr(&st->error, 2);
                st->epoch = st->epoch + 1u;
            }
            return;
        }
        if (p < st->prompt_len)
            tok = prompt[p];
        else
            tok = spec_argmax(L.partials[0], np, sh);
        if (threadIdx.x == 0) {
            if (tok < 0 || tok >= st->vocab) {
                atomicOr(&st->error, 1);
                tok = 0;
            }
            tok_s = tok;
            tokens[p] = tok;
            st->cur_pos = p;
            st->next_pos = p + 1;
            st->epoch = st->epoch + 1u;  // (no granule is written in a verify step; the epoch only moves on)
        }
    } else if (threadIdx.x == 0) {
        tok = draft[lane - 1];
        if (tok < 0 || tok >= L.st[0]->vocab) {  // (only `vocab` of the engine's state is read here)
            atomicOr(&L.st[lane]->error, 1);
            tok = 0;
        }
        tok_s = tok;
    }
    __syncthreads();
    tok = tok_s;
    const TT* row = table + (size_t)tok * hidden;
    float* x = L.x[lane];
    long long* r0 = L.res0[lane];
    long long* xa = L.xacc[lane];
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = to_f32(row[i]);
        x[i] = v;
        r0[i] = to_fixed(v);
        if (xa) xa[i] = to_fixed(v);
    }
}

// One workgroup. g_i = argmax of lane i's partials (ties to the lowest id, as finalize reads
// them); a = the longest accepted prefix. Then the engine's state is made that of a + 1 plain
// steps: positions, tokens p + 1 .. p + a (p was recorded by spec_start), lane a's partials,
// logits and hidden state in the engine's buffers, the lanes' error words or-ed into the
// engine's. out = {a, g_a, error}.
__global__ __launch_bounds__(kSpecT) void spec_commit_kernel(SpecLanes L, int np, int32_t* tokens,
                                                             const int32_t* draft, int hidden, int vocab_rows,
                                                             int max_seq, int* out) {
    __shared__ unsigned long long sh[kSpecT / 64];
    __shared__ int g_s[kAttnRowsMax];
    for (int i = 0; i < L.m; ++i) {
        const int g = spec_argmax(L.partials[i], np, sh);
        if (threadIdx.x == 0) g_s[i] = g;
    }
    __syncthreads();  // (also: every read of lane 0's partials is done before they are overwritten)
    int a = 0;
    while (a < L.m - 1 && draft[a] == g_s[a]) ++a;
    DecodeState* st = L.st[0];
    if (threadIdx.x == 0) {
        const int p = st->cur_pos;
        int err = 0;
        for (int i = 1; i < L.m; ++i) {
            err |= L.st[i]->error;
            L.st[i]->error = 0;
        }
        if (err) atomicOr(&st->error, err);
        if (p + a < max_seq) {
            for (int j = 1; j <= a; ++j) tokens[p + j] = draft[j - 1];
            st->cur_pos = p + a;
            st->next_pos = p + a + 1;
        }
        out[0] = a;
        out[1] = g_s[a];
        out[2] = st->error;
    }
    if (a > 0) {
        const unsigned long long* ps = L.partials[a];
        unsigned long long* pd = L.partials[0];
        for (int i = threadIdx.x; i < np; i += blockDim.x) pd[i] = ps[i];
        const float* ls = L.logits[a];
        float* ld = L.logits[0];
        for (int i = threadIdx.x; i < vocab_rows; i += blockDim.x) ld[i] = ls[i];
        const float* xs = L.x[a];
        float* xd = L.x[0];
        for (int i = threadIdx.x; i < hidden; i += blockDim.x) xd[i] = xs[i];
    }
}

}  // namespace

int Engine::set_speculation(int max_draft) {
    LLMI_REQUIRE(max_draft >= 0 && max_draft <= kAttnRowsMax - 1, "set_speculation: max_draft must be in [0, 7]");
    if (max_draft > 0) LLMI_TRY(refuse("set_speculation", kModeSpec));
    LLMI_TRY(spec_graphs.drop(stream));  // (the token steps stay: no lane is part of them)
    if (max_draft > 0 && !spec_draft) {
        LLMI_HIP(hipMalloc(&spec_draft, (kAttnRowsMax + 4) * sizeof(int32_t)));
        LLMI_HIP(hipMemset(spec_draft, 0, (kAttnRowsMax + 4) * sizeof(int32_t)));
    }
    while ((int)lanes.size() < max_draft) {
        std::unique_ptr<Engine> l(new Engine());
        l->kv_from = this;
        LLMI_TRY(l->init(c, device, nullptr, stream, this, false));
        lanes.push_back(std::move(l));
    }
    spec_max = max_draft;
    return LLMI_OK;
}

// one verify step of m = 2..8 rows; rec_nact = the split count of the last row's position
int Engine::record_verify(int m) {
    auto lane = [&](int i) -> Engine& { return i == 0 ? *this : *lanes[i - 1]; };
    std::vector<Engine*> es;
    for (int i = 0; i < m; ++i) es.push_back(&lane(i));
    // one multi-row GEMV from the lanes' own single-row arguments (no debug stamps)
    auto spec_rows = [&](auto&& args_of) { return gemv_rows_of(es, stream, args_of, false); };
    SpecLanes L;
    L.m = m;
    for (int i = 0; i < kAttnRowsMax; ++i) {
        Engine& e = lane(i < m ? i : 0);
        L.x[i] = e.x; L.res0[i] = e.res[0]; L.xacc[i] = seed_from_down() ? e.xacc : nullptr;
        L.partials[i] = e.partials; L.logits[i] = e.logits; L.st[i] = e.st;
    }
    int32_t* out = spec_draft + kAttnRowsMax;
    if (edt == LLMI_F16)
        hipLaunchKernelGGL(spec_start_kernel<__half>, dim3(m), dim3(kSpecT), 0, stream, L, prompt, lm_grid, tokens,
                           spec_draft, (const __half*)embed, c.hidden, c.max_seq);
    else
        hipLaunchKernelGGL(spec_start_kernel<float>, dim3(m), dim3(kSpecT), 0, stream, L, prompt, lm_grid, tokens,
                           spec_draft, (const float*)embed, c.hidden, c.max_seq);
    LLMI_HIP(hipGetLastError());
    for (int l = 0; l < c.layers; ++l) {
        LLMI_TRY(spec_rows([&](Engine& e) { return e.qkv_args(l); }));
        AttnRowsArgs at;
        OprojRowsArgs o;
        at.m = o.m = m;
        for (int i = 0; i < m; ++i) {
            Engine& e = lane(i);
            e.rec_nact = rec_nact;
            const AttnArgs ai = e.attn_args(l);
            if (i == 0) {
                at.a = ai;
                o.a = o_args(l);
            }
            AttnRow& r = at.row[i];
            r.qkv = ai.qkv; r.workspace = ai.workspace; r.xacc = ai.xacc;
            r.resid = ai.resid; r.resid_fixed = ai.resid_fixed; r.resid_scale = ai.resid_scale;
            o.row[i] = r;
            o.row[i].xacc = e.xacc;  // (ai.xacc is null when the down GEMV seeded it)
        }
        at.a.stamps = nullptr;
        o.a.stamps = nullptr;
        LLMI_TRY(attn_rows_launch(at, stream));
        LLMI_TRY(oproj_rows_launch(o, stream));
        LLMI_TRY(spec_rows([&](Engine& e) { return e.gu_args(l); }));
        LLMI_TRY(spec_rows([&](Engine& e) { return e.down_args(l); }));
    }
    LLMI_TRY(spec_rows([&](Engine& e) { return e.lm_args(); }));
    hipLaunchKernelGGL(spec_commit_kernel, dim3(1), dim3(kSpecT), 0, stream, L, lm_grid, tokens, spec_draft, c.hidden,
                       vl, c.max_seq, out);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

int Engine::verify(const int32_t* draft, int n_draft, int use_graph, int* n_accepted, int* next_token) {
    LLMI_REQUIRE(prompt_len > 0, "verify: set_prompt first");
    LLMI_REQUIRE(n_accepted != nullptr, "verify: null n_accepted");
    LLMI_REQUIRE(host_next_pos >= prompt_len, "verify: the prompt is not consumed yet (decode or prefill it first)");
    LLMI_REQUIRE(n_draft >= 0 && n_draft <= spec_max, "verify: n_draft must be in [0, max_draft] (set_speculation)");
    LLMI_REQUIRE(n_draft == 0 || draft != nullptr, "verify: null draft");
    LLMI_REQUIRE(host_next_pos + n_draft + 1 <= c.max_seq, "verify: would run past max_seq");
    for (int i = 0; i < n_draft; ++i)
        LLMI_REQUIRE(draft[i] >= 0 && draft[i] < c.vocab, "verify: draft id out of range");
    if (n_draft > 0) LLMI_TRY(refuse("set_speculation", kModeSpec));
    const int m = n_draft + 1;
    int out[3] = {0, 0, 0};
    if (m == 1) {  // the engine's own single-row step
        LLMI_TRY(decode(1, use_graph));
        LLMI_TRY(finalize_launch(st, partials, lm_grid, tokens, c.max_seq, stream));
        LLMI_HIP(hipStreamSynchronize(stream));
        DecodeState h;
        LLMI_HIP(hipMemcpy(&h, st, sizeof(h), hipMemcpyDeviceToHost));
        LLMI_HIP(hipMemcpy(&out[1], tokens + host_next_pos, 4, hipMemcpyDeviceToHost));
        out[2] = h.error;
    } else {
        LLMI_HIP(hipMemcpyAsync(spec_draft, draft, (size_t)n_draft * 4, hipMemcpyHostToDevice, stream));
        rec_nact = nact_of(host_next_pos + n_draft);
        if (use_graph) {
            hipGraphExec_t step = nullptr;
            LLMI_TRY(spec_graphs.get({m, rec_nact}, stream, [&]() { return record_verify(m); }, &step));
            LLMI_HIP(hipGraphLaunch(step, stream));
        } else {
            LLMI_TRY(record_verify(m));
        }
        LLMI_HIP(hipStreamSynchronize(stream));
        LLMI_HIP(hipMemcpy(out, spec_draft + kAttnRowsMax, sizeof(out), hipMemcpyDeviceToHost));
        LLMI_REQUIRE(out[0] >= 0 && out[0] <= n_draft, "verify: the device reported an impossible accepted count");
        host_next_pos += out[0] + 1;
    }
    LLMI_REQUIRE(out[2] == 0, "verify: device error flag " + error_flag_text(out[2]));
    *n_accepted = out[0];
    if (next_token) *next_token = out[1];
    return LLMI_OK;
}

int lookup_draft(const int32_t* ids, int n, int ngram_max, int ngram_min, int max_draft, int32_t* out, int* n_out) {
    LLMI_REQUIRE(ids && out && n_out, "lookup_draft: null pointer");
    LLMI_REQUIRE(n >= 0 && ngram_min >= 1 && ngram_max >= ngram_min, "lookup_draft: need n >= 0 and 1 <= ngram_min <= ngram_max");
    LLMI_REQUIRE(max_draft >= 0 && max_draft <= kAttnRowsMax - 1, "lookup_draft: max_draft must be in [0, 7]");
    *n_out = 0;
    for (int g = std::min(ngram_max, n - 1); g >= ngram_min; --g) {
        const int32_t* suf = ids + n - g;
        for (int s = n - g - 1; s >= 0; --s) {  // the largest matching start wins
            if (std::memcmp(ids + s, suf, (size_t)g * 4) != 0) continue;
            const int end = std::min(n, s + g + max_draft);
            for (int i = s + g; i < end; ++i) out[(*n_out)++] = ids[i];
            return LLMI_OK;
        }
    }
    return LLMI_OK;
}

int Engine::generate_lookup(int n_steps, int max_draft, int ngram_max, int ngram_min, int use_graph,
                            llmi_spec_stats* stats) {
    LLMI_REQUIRE(n_steps >= 0, "generate_lookup: n_steps must be >= 0");
    LLMI_REQUIRE(max_draft >= 0 && max_draft <= spec_max, "generate_lookup: max_draft must be in [0, set_speculation's]");
    LLMI_REQUIRE(ngram_min >= 1 && ngram_max >= ngram_min, "generate_lookup: need 1 <= ngram_min <= ngram_max");
    LLMI_REQUIRE(prompt_len > 0 && host_next_pos >= prompt_len, "generate_lookup: the prompt is not consumed yet");
    LLMI_REQUIRE(host_next_pos + n_steps <= c.max_seq, "generate_lookup: would run past max_seq");
    llmi_spec_stats st_{0, 0, 0};
    // the sequence so far and the pending token (position host_next_pos), read once
    std::vector<int32_t> hist((size_t)c.max_seq + 1);
    int valid = 0;
    if (n_steps > 0) {
        LLMI_TRY(tokens_out(hist.data(), c.max_seq + 1, &valid));
        LLMI_REQUIRE(valid == host_next_pos + 1, "generate_lookup: the token history is short");
    }
    int remaining = n_steps;
    while (remaining > 0) {
        const int p = host_next_pos;
        int32_t draft[kAttnRowsMax];
        int nd = 0;
        const int cap = std::min(std::min(max_draft, remaining - 1), c.max_seq - p - 1);
        if (cap > 0) LLMI_TRY(lookup_draft(hist.data(), p + 1, ngram_max, ngram_min, cap, draft, &nd));
        int a = 0, next = 0;
        LLMI_TRY(verify(draft, nd, use_graph, &a, &next));
        for (int j = 0; j < a; ++j) hist[p + 1 + j] = draft[j];
        hist[p + a + 1] = next;
        st_.verify_steps += 1;
        st_.drafted += nd;
        st_.accepted += a;
        remaining -= a + 1;
    }
    if (stats) *stats = st_;
    return LLMI_OK;
}

// ------------------------------------------------------------ a draft engine proposes
// tokens[from .. from + n) read back narrowly (the pending token is finalized first), with the
// device error word: all a draft loop ever reads of an engine
int Engine::read_ids(int from, int n, int32_t* out) {
    if (host_next_pos >= prompt_len && host_next_pos <= c.max_seq)
        LLMI_TRY(finalize_launch(st, partials, lm_grid, tokens, c.max_seq, stream));
    LLMI_HIP(hipStreamSynchronize(stream));
    int err = 0;
    LLMI_HIP(hipMemcpy(&err, &st->error, sizeof(int), hipMemcpyDeviceToHost));
    LLMI_REQUIRE(err == 0, "generate_draft: the draft's device error flag " + error_flag_text(err));
    LLMI_REQUIRE(from >= 0 && n >= 0 && from + n <= c.max_seq + 1, "generate_draft: ids out of range");
    if (n > 0) LLMI_HIP(hipMemcpy(out, tokens + from, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

// This (draft) engine takes the target's sequence hist[0 .. p] (p: the target's next position,
// hist[p] its pending token): the longest prefix it has already consumed with the same ids is
// kept, the rest forced, and every forced position but p run -- next position p afterwards.
int Engine::draft_catch_up(const int32_t* hist, int p, int use_prefill, int use_graph) {
    int m = 0;
    if (prompt_len > 0) {
        const int have = std::min(host_next_pos, p);  // (position p is always forced)
        std::vector<int32_t> own((size_t)have);
        if (have > 0) LLMI_TRY(read_ids(0, have, own.data()));
        while (m < have && own[m] == hist[m]) ++m;
        LLMI_TRY(edit(m, hist + m, p + 1 - m));
    } else {
        LLMI_TRY(set_prompt(hist, p + 1));
    }
    const int rows = p - m;
    if (rows == 0) return LLMI_OK;
    if (use_prefill && rows > 1 && wdt != LLMI_I4) return prefill(rows, 2);
    return decode(rows, use_graph);
}

int Engine::generate_draft(Engine& d, int n_steps, int max_draft, int draft_prefill, int use_graph,
                           llmi_spec_stats* stats) {
    LLMI_REQUIRE(n_steps >= 0, "generate_draft: n_steps must be >= 0");
    LLMI_REQUIRE(&d != this, "generate_draft: the draft is the target itself");
    LLMI_REQUIRE(d.c.tp_world == 1 && !d.grouped && !d.kv_from, "generate_draft: the draft must be a single-rank engine");
    LLMI_REQUIRE(d.decode_mode == 0, "generate_draft: the draft runs decode mode 0 (the ring mode has no edit)");
    LLMI_REQUIRE(d.c.vocab == c.vocab, "generate_draft: the draft's vocab differs from the target's");
    LLMI_REQUIRE(d.device == device, "generate_draft: the draft is on another device");
    LLMI_REQUIRE(d.c.max_seq >= c.max_seq, "generate_draft: the draft's max_seq is smaller than the target's");
    LLMI_TRY(refuse("generate_draft: the target", kModeSpec));
    LLMI_REQUIRE(max_draft >= 0 && max_draft <= spec_max, "generate_draft: max_draft must be in [0, set_speculation's]");
    LLMI_REQUIRE(prompt_len > 0 && host_next_pos >= prompt_len, "generate_draft: the target's prompt is not consumed yet");
    LLMI_REQUIRE(host_next_pos + n_steps <= c.max_seq, "generate_draft: would run past max_seq");
    llmi_spec_stats st_{0, 0, 0};
    if (stats) *stats = st_;
    if (n_steps == 0) return LLMI_OK;
    // the target's sequence and its pending token (position host_next_pos), read once
    std::vector<int32_t> hist((size_t)c.max_seq + 1);
    int valid = 0;
    LLMI_TRY(tokens_out(hist.data(), c.max_seq + 1, &valid));
    LLMI_REQUIRE(valid == host_next_pos + 1, "generate_draft: the token history is short");
    LLMI_TRY(d.draft_catch_up(hist.data(), host_next_pos, draft_prefill, use_graph));
    int remaining = n_steps;
    while (remaining > 0) {
        const int p = host_next_pos;
        const int k = std::max(0, std::min(std::min(max_draft, remaining - 1), c.max_seq - p - 1));
        int32_t prop[kAttnRowsMax];
        if (k > 0) {  // the forced ids it has not consumed yet, then k - 1 of its own: ids p + 1 .. p + k
            LLMI_TRY(d.decode(p + k - d.host_next_pos, use_graph));
            LLMI_TRY(d.read_ids(p + 1, k, prop));
        }
        int a = 0, next = 0;
        LLMI_TRY(verify(prop, k, use_graph, &a, &next));
        for (int j = 0; j < a; ++j) hist[p + 1 + j] = prop[j];
        hist[p + a + 1] = next;
        // the draft drops what was rejected and takes the target's token: one id, or two when
        // every proposal was accepted (its own pending id, now consumed by the target, and g)
        const int last = std::min(p + a + 1, d.c.max_seq - 1);
        const int keep = std::min(last, d.host_next_pos);
        LLMI_TRY(d.edit(keep, hist.data() + keep, last - keep + 1));
        st_.verify_steps += 1;
        st_.drafted += k;
        st_.accepted += a;
        remaining -= a + 1;
    }
    if (stats) *stats = st_;
    return LLMI_OK;
}

}  // namespace llmi
