// The token step of the decode engine: the launch arguments, the recorded step and its
// graph, the TP exchange, the ring layer, and the sampling / logprob / option setters.
// See engine.h.
#include "engine.h"
#include "rules_host.h"
#include "xchg_impl.h"

namespace llmi {

// ---------------------------------------------------------- one token
GemvArgs Engine::lm_args(bool from_x) const {
    GemvArgs a;
    a.stamps = stamp_ptr();
    a.w = lm_head;
    a.w_dtype = edt;
    a.n_rows = vl;
    a.k = c.hidden;
    if (from_x) {
        a.x = x;
    } else {
        a.x_fixed = res[c.layers % 2];  // final residual; fp32 copy to x by workgroup 0
        a.x_out = x;
    }
    a.gamma = final_norm;
    a.g_dtype = edt;
    a.eps = c.rms_eps;
    a.epi = EPI_ARGMAX;
    a.y = logits;
    a.partials = partials;
    a.idx_base = (uint32_t)(c.tp_rank * vl);
    return a;
}

// K split inside the workgroup for row-group counts that leave CUs idle or doubled with
// one group per wave (a TP rank's q/k/v and gate_up): 4 waves per group below one
// workgroup per CU, 2 below two; TP 1 shapes never qualify (tp_world 1 keeps kpar off so
// its sums stay bitwise those of the fixtures' runs)
int Engine::kpar_of(int groups) const {
    if (c.tp_world == 1 || kpar_off) return 0;
    // the K-parted kernel stages x for k <= 5120 and splits a row's 16-B chunks evenly
    // (a wider model must fall back to kpar 0, not fail the launch)
    const int epl = wdt == LLMI_I8 ? 16 : wdt == LLMI_F16 ? 8 : 4;  // (int4: tp_world 1 only, returned above)
    if (c.hidden > 5120 || c.hidden % epl != 0) return 0;
    const int cus = n_cu > 0 ? n_cu : 256;
    const int blocks = (groups + 3) / 4;
    const int kp = blocks < cus ? 4 : blocks < 2 * cus ? 2 : 0;
    return kp > 0 && (c.hidden / epl) % kp == 0 ? kp : 0;
}

GemvArgs Engine::qkv_args(int l) const {
    const Layer& L = layers[l];
    GemvArgs a;
    a.stamps = stamp_ptr();
    a.w = L.qkv; a.scales = L.qkv_s; a.w_dtype = wdt;
    a.n_rows = ql + 2 * kvrows; a.k = c.hidden;
    a.x_fixed = res[l % 2]; a.gamma = L.attn_norm; a.g_dtype = edt; a.eps = c.rms_eps;
    a.epi = EPI_STORE; a.y = qkv_buf;
    a.kpar = kpar_of((a.n_rows + 1) / 2);
    return a;
}
AttnArgs Engine::attn_args(int l) const {
    AttnArgs a;
    a.stamps = stamp_ptr();
    a.qkv = qkv_buf;
    a.k_cache = kv_layer(l, 0);
    a.v_cache = kv_layer(l, 1);
    a.cache_dtype = c.kv_dtype;
    a.k_scale = kv_scale_layer(l, 0);
    a.v_scale = kv_scale_layer(l, 1);
    a.max_seq = c.max_seq;
    a.pos_dev = &st->cur_pos;
    a.heads = hl; a.kv_heads = kvl; a.head_dim = c.head_dim;
    a.rope = 1; a.rope_base = c.rope_base; a.rope_tab = rope_tab;
    a.direct_out = 0;  // partials -> attn_oproj
    a.xacc = xacc;
    a.resid_fixed = res[l % 2];
    a.resid_scale = (c.tp_rank == 0) ? 1.f : 0.f;  // rank 0 carries the residual into the all-reduce
    a.hidden = c.hidden;
    a.out = attn_out; a.workspace = attn_ws;
    a.nact = rec_nact;
    a.err = &st->error;
    if (seed_from_down()) a.xacc = nullptr;  // layer l - 1's down (layer 0: step_start) seeded xacc already
    return a;
}
OprojArgs Engine::o_args(int l) const {
    const Layer& L = layers[l];
    OprojArgs a;
    a.stamps = stamp_ptr();
    a.w = L.o; a.scales = L.o_s; a.w_dtype = odt();  // (int4 engines: W_o is W8A16)
    a.head_major = 0;
    a.n_rows = c.hidden; a.ldw = ql;
    a.heads = hl; a.head_dim = c.head_dim; a.max_seq = c.max_seq;
    a.pos_dev = &st->cur_pos;
    a.workspace = attn_ws; a.xacc = xacc;
    a.nact = rec_nact;
    a.err = &st->error;
    return a;
}
GemvArgs Engine::gu_args(int l) const {
    const Layer& L = layers[l];
    GemvArgs a;
    a.stamps = stamp_ptr();
    a.w = L.gu; a.scales = L.gu_s; a.w_dtype = wdt;
    a.n_rows = 2 * il; a.k = c.hidden;
    a.x_fixed = xacc;  // residual after attention (fixed point)
    // (no fp32 copy into x here: the lm_head launch writes the final hidden state there, and
    // nothing reads a mid-layer copy -- it was 16 KB of stores on workgroup 0 every layer)
    // hand the mid-layer residual to the layer output accumulator (rank 0 carries it) --
    // unless the down GEMV writes each output row itself (down_single)
    if (!down_single()) {
        a.seed_src = xacc; a.seed_dst = res[(l + 1) % 2]; a.seed_n = c.hidden;
        a.seed_keep = c.tp_rank == 0 ? 1 : 0;
    }
    a.gamma = L.ffn_norm; a.g_dtype = edt; a.eps = c.rms_eps;
    a.epi = EPI_SILU_MUL; a.pair_off = il; a.y = act;
    a.kpar = kpar_of(il);
    return a;
}
GemvArgs Engine::down_args(int l) const {
    const Layer& L = layers[l];
    GemvArgs a;
    a.stamps = stamp_ptr();
    a.w = L.down; a.scales = L.down_s; a.w_dtype = wdt;
    a.n_rows = c.hidden; a.k = il; a.x = act;
    a.epi = EPI_ATOMIC; a.yacc = res[(l + 1) % 2];
    // int8 rows are half the bytes of fp16 ones: K slices keep the loads per row in
    // flight and the x image per workgroup small (exact: int64 atomics)
    a.ksplit = down_ksplit();
    if (down_single()) {  // one producer per row: x_{l+1}[r] = xmid[r] + fixed(down_r), no seed, no atomic
        a.yacc_single = 1;
        a.yacc_base = c.tp_rank == 0 ? xacc : nullptr;  // the other TP ranks carry no residual
        // single rank: the same row also seeds the next layer's o_proj sum (xacc), so that
        // layer's attention writes no seed (seed_from_down)
        if (seed_from_down()) a.yacc_copy = xacc;
    }
    return a;
}
int Engine::down_ksplit() const {
    return (wdt == LLMI_I8 && il % (16 * LLMI_I8_DOWN_KSPLIT) == 0) ? LLMI_I8_DOWN_KSPLIT
           : (wdt == LLMI_F16 && il % (8 * LLMI_F16_DOWN_KSPLIT) == 0) ? LLMI_F16_DOWN_KSPLIT
                                                                       : 1;
}
// the down GEMV writes its rows itself (round 6) when K is not split
bool Engine::down_single() const { return down_ksplit() == 1; }
// ... and on a single rank also the next layer's o_proj seed (with TP the seed must be the
// all-reduced residual, which only exists after the exchange)
bool Engine::seed_from_down() const { return down_single() && c.tp_world == 1 && !grouped; }
// the fused q/k/v + attention launch's granule tags: the GEMV part tags what it writes with
// (epoch, layer l), the attention part waits for that tag
void Engine::tag_qkv(GemvArgs& q, AttnArgs& at, int l) const {
    q.y_tag = qtag; q.tag_epoch = &st->epoch; q.tag_layer = (unsigned)l;
    at.qkv_tag = qtag; at.tag_epoch = &st->epoch; at.tag_layer = (unsigned)l;
}

// One token = start, L x (attention phase | reduce xacc, ffn phase | reduce x),
// head | reduce partials. The phases are separate so that an in-process
// group (struct Group) can interleave its ranks between the reductions.
int Engine::rec_start() {
    return step_start_launch(st, prompt, partials, lm_grid, tokens, embed, edt, c.hidden, x, res[0], c.max_seq,
                             nullptr, 0, stream, seed_from_down() ? xacc : nullptr);
}
int Engine::rec_attn(int l) {
    GemvArgs q = qkv_args(l);
    AttnArgs at = attn_args(l);
    if (qa_fuse && qtag && l < 128) {
        GemvArgs qf = q;
        qf.kpar = 0;  // the fused GEMV part streams a row group per wave (kpar: +0.3 % alone at TP 8)
        AttnArgs af = at;
        tag_qkv(qf, af, l);
        OprojArgs o = o_args(l);
        if (qa_o && !tail_mode && qkv_attn_o_supported(qf, af, o))  // q/k/v, attention and o_proj: one launch
            return qkv_attn_o_launch(qf, af, &o, stream);
        if (qkv_attn_supported(qf, af)) return rec_oproj(qkv_attn_launch(qf, af, stream), o);  // one launch
        return rec_oproj(gemv_launch(q, stream), o, &at);
    }
    LLMI_TRY(gemv_launch(q, stream));
    return rec_oproj(LLMI_OK, o_args(l), &at);
}
// the layer's o_proj launch (after the attention launch when `at` is given)
int Engine::rec_oproj(int prev, OprojArgs o, const AttnArgs* at) {
    LLMI_TRY(prev);
    if (at) LLMI_TRY(attn_decode_launch(*at, stream));
    if (tail_mode) {  // the o_proj launch pushes (and reduces) xacc itself
        o.xt = xchg_args(xacc, c.hidden, 0, tail_mode);
        o.xt_cnt = xt_cnt;
    }
    return attn_oproj_launch(o, stream);
}
int Engine::rec_ffn(int l) {
    LLMI_TRY(gemv_launch(gu_args(l), stream));
    GemvArgs d = down_args(l);
    if (tail_mode) {  // the down launch pushes (and reduces) the layer output itself
        d.xt = xchg_args(res[(l + 1) % 2], c.hidden, 0, tail_mode);
        d.xt_cnt = xt_cnt;
    }
    return gemv_launch(d, stream);
}
int Engine::rec_head(bool from_x) {
    GemvArgs h = lm_args(from_x);
    if (tail_mode) {  // the lm_head launch max-reduces the argmax keys itself
        h.xt = xchg_args(partials, lm_grid, 2, tail_mode);
        h.xt_cnt = xt_cnt;
    }
    LLMI_TRY(gemv_launch(h, stream));
    return rec_sample();
}
// the sampled id replaces the argmax partials: the nucleus sampler over the whole row
// (history tokens[0 .. cur_pos]: step_start / prefill_finish have written them), or
// top-K of this token's logits and the reference's pick
int Engine::rec_sample() {
    LLMI_TRY(rec_pick());
    return rec_logprob();
}
// With logit rules on, their launch comes first: it leaves the processed row in lr_out and its
// argmax as the only non-zero partial (the greedy pick), and a sampler then reads lr_out.
int Engine::rec_pick() {
    const float* row = logits;
    if (rules_on()) {
        LLMI_TRY(engine_logit_rules_launch(st, logits, c.vocab, lr_bias_on ? lr_bias : nullptr, lr_allowed, tokens,
                                           lr_count_prompt, lr_presence, lr_frequency, lr_out, partials, lm_grid,
                                           stream));
        row = lr_out;
    }
    if (nuc_on)
        return engine_nucleus_launch(st, row, c.vocab, tokens, nuc.repetition_penalty, nuc.temperature,
                                     nuc.top_k, nuc.top_p, nuc.seed, partials, lm_grid, stream);
    if (sample_k == 0) return LLMI_OK;
    LLMI_TRY(topk_launch(row, LLMI_F32, 1, c.vocab, sample_k, samp_ids, samp_vals, stream));
    return sample_pick_launch(st, samp_ids, samp_vals, sample_k, sample_seed, partials, lm_grid, stream);
}
// record cur_pos + 1: the raw row's logprob of the token step_start will pick there (the
// prompt's, or the one the partials name now that the sampler has run) and the top-n
int Engine::rec_logprob() {
    if (lp_top < 0) return LLMI_OK;
    return engine_logprob_launch(st, logits, c.vocab, prompt, partials, lm_grid, c.max_seq, lp_top, lp_tok(),
                                 lp_ids(), lp_tlp(), stream);
}

// ------------------------------------------------- TP exchange (config 4)
// The per-token collectives: int64 sum of the residual partials (op 0) or uint64 max of
// the argmax keys (op 2), over RCCL or the one-shot peer exchange.
int Engine::alloc_xchg() {
    if (inbox) return LLMI_OK;
    const int W = c.tp_world;
    LLMI_REQUIRE(W <= kXchgMaxWorld, "xchg: the one-shot exchange takes at most 8 ranks");
    xchg_cap_n = std::max(c.hidden, lm_grid);
    xchg_cap_n += xchg_cap_n & 1;
    LLMI_REQUIRE(xchg_cap_n <= kXchgSlice * kXchgMaxSlices, "xchg: hidden / lm_head partials exceed the inbox");
    const size_t bytes = xchg_inbox_bytes(W, xchg_cap_n);
    LLMI_HIP(hipExtMallocWithFlags(reinterpret_cast<void**>(&inbox), bytes, hipDeviceMallocUncached));
    LLMI_HIP(hipMemset(inbox, 0, bytes));
    LLMI_HIP(hipMalloc(&xchg_ep, kXchgMaxSlices * sizeof(unsigned long long)));
    LLMI_HIP(hipMemset(xchg_ep, 0, kXchgMaxSlices * sizeof(unsigned long long)));
    LLMI_HIP(hipMalloc(&peers_dev, (size_t)W * sizeof(char*)));
    LLMI_HIP(hipMalloc(&xt_cnt, xchg_detail::kTailWords * sizeof(unsigned)));
    LLMI_HIP(hipMemset(xt_cnt, 0, xchg_detail::kTailWords * sizeof(unsigned)));
    return LLMI_OK;
}
// every rank's inbox base, in rank order (peers[rank] must be this rank's own inbox)
int Engine::set_peers(const std::vector<char*>& p) {
    LLMI_REQUIRE((int)p.size() == c.tp_world && p[c.tp_rank] == inbox, "xchg: bad peer table");
    LLMI_HIP(hipMemcpy(peers_dev, p.data(), p.size() * sizeof(char*), hipMemcpyHostToDevice));
    return LLMI_OK;
}
XchgArgs Engine::xchg_args(void* buf, int n, int op, int mode) const {
    XchgArgs a;
    a.buf = static_cast<long long*>(buf);
    a.n = n;
    a.op = op;
    a.rank = c.tp_rank;
    a.world = c.tp_world;
    a.peers = peers_dev;
    a.ep = xchg_ep;
    a.err = &st->error;
    a.mode = mode;
    a.cap_n = xchg_cap_n;
    a.cap_w = c.tp_world;
    a.loop = xchg_loop;
    return a;
}
int Engine::exchange(void* buf, int n, int op) {
    if (xchg_mode == 1) return xchg_launch(xchg_args(buf, n, op, 3), stream);
    if (xchg_mode == 2) return LLMI_OK;  // the producing launch's tail did it
    if (!comm) return LLMI_OK;
    const ncclResult_t r = op == 0 ? ncclAllReduce(buf, buf, n, ncclInt64, ncclSum, comm, stream)
                                   : ncclAllReduce(buf, buf, n, ncclUint64, ncclMax, comm, stream);
    LLMI_REQUIRE(r == ncclSuccess, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    return LLMI_OK;
}
int Engine::set_exchange(int mode) {
    LLMI_REQUIRE(mode >= 0 && mode <= 2,
                 "set_exchange: mode must be 0 (RCCL), 1 (one-shot peer exchange) or 2 (fused into the producers)");
    LLMI_REQUIRE(!grouped, "set_exchange: a group rank's exchange is its group's");
    LLMI_REQUIRE(mode == 0 || (inbox && peers_ready), "set_exchange: open the peer exchange first (xchg_open)");
    LLMI_TRY(invalidate());
    xchg_mode = mode;
    tail_mode = mode == 2 ? 3 : 0;
    return LLMI_OK;
}
// ------------------------------------------------- captured steps and modes
// Whatever changes a recorded step's launches or their arguments ends here: this engine's token
// and verify steps are dropped, and so are the captured steps of the owner that holds this
// engine's launches (a slot's batch, a verify lane's engine). Each drop synchronises only where
// there is something to drop: a replay may still be in flight.
int Engine::invalidate() {
    LLMI_TRY(graphs.drop(stream));
    LLMI_TRY(spec_graphs.drop(stream));
    if (owner_graphs) LLMI_TRY(owner_graphs->drop(stream));
    return kv_from ? kv_from->invalidate() : LLMI_OK;
}

// Which mode refuses which: `turning_on` is refused with `why` while `on` is on, the first row
// that applies. The modes fixed at creation can only be the `on` side. Every pair of modes that
// setters turn on is listed in both directions (checked below).
namespace {
struct Refusal {
    Mode turning_on, on;
    int code;
    const char* why;
};
constexpr int kU = LLMI_EUNSUPPORTED, kI = LLMI_EINVAL;
constexpr Refusal kRefusals[] = {
    {kModeSlot, kModeTp, kU, "tensor-parallel batches are not built (tp_world must be 1)"},
    {kModeSlot, kModeInt4, kU, "int4 weights are not built into the multi-row GEMV (use an Engine)"},
    {kModeTp, kModeInt4, kU, "int4 weights run on a single-rank engine only (no tensor parallel)"},
    {kModeRing, kModeInt4, kU, "the ring layer streams fp16 weights; int4 engines run mode 0"},
    {kModeRing, kModeSpec, kU, "speculation is on (the ring layer has no verify step)"},
    {kModeRing, kModeRules, kU, "logit rules are on (not built into the ring mode; clear_logit_rules first)"},
    // (the two kI rows keep the condition text that LLMI_REQUIRE appends to such a message)
    {kModeTopK, kModeTp, kI,
     "sampling needs the full logits (tp_world 1) (k == 0 || (c.tp_world == 1 && !grouped))"},
    {kModeTopK, kModeSpec, kU, "speculation is on (greedy only; set_speculation 0 first)"},
    {kModeNucleus, kModeTp, kI, "sampling needs the full logits (tp_world 1) (c.tp_world == 1 && !grouped)"},
    {kModeNucleus, kModeSpec, kU, "speculation is on (greedy only; set_speculation 0 first)"},
    {kModeLogprobs, kModeTp, kU, "logprobs need the full logits row (tp_world 1, no group rank)"},
    {kModeLogprobs, kModeSpec, kU, "speculation is on (the verify step records none; set_speculation 0 first)"},
    {kModeRules, kModeTp, kU, "the rules need the full logits row (tp_world 1, no group rank)"},
    {kModeRules, kModeSpec, kU, "speculation is on (the verify step applies no rules; set_speculation 0 first)"},
    {kModeRules, kModeRing, kU, "the ring decode mode is on (set_decode_mode 0 first)"},
    {kModeSpec, kModeTp, kU, "tensor-parallel ranks and group ranks are not built (tp_world must be 1)"},
    {kModeSpec, kModeInt4, kU, "int4 weights are not built into the multi-row GEMV"},
    {kModeSpec, kModeKv8, kU, "an int8 KV cache is not built into the multi-row attention"},
    {kModeSpec, kModeRing, kU, "the ring decode mode has no verify step (set_decode_mode 0)"},
    {kModeSpec, kModeTopK, kU, "a sampler is active (speculative sampling is not built; greedy only)"},
    {kModeSpec, kModeNucleus, kU, "a sampler is active (speculative sampling is not built; greedy only)"},
    {kModeSpec, kModeLogprobs, kU, "logprobs are on (the verify step records none)"},
    {kModeSpec, kModeRules, kU, "logit rules are on (the verify step applies none; clear_logit_rules first)"},
};
constexpr bool refused(Mode turning_on, Mode on) {
    for (const Refusal& r : kRefusals)
        if (r.turning_on == turning_on && r.on == on) return true;
    return false;
}
constexpr bool refusals_symmetric() {
    for (const Refusal& r : kRefusals)
        if (r.on >= kModeRing && !refused(r.on, r.turning_on)) return false;
    return true;
}
static_assert(refusals_symmetric(), "two modes that setters turn on refuse each other in one direction only");
}  // namespace

unsigned Engine::config_modes(const llmi_config& cfg) {
    return (cfg.tp_world != 1 ? 1u << kModeTp : 0) | (cfg.weight_dtype == LLMI_I4 ? 1u << kModeInt4 : 0) |
           (cfg.kv_dtype == LLMI_I8 ? 1u << kModeKv8 : 0);
}
unsigned Engine::modes() const {
    return config_modes(c) | (grouped ? 1u << kModeTp : 0) | (owner_graphs ? 1u << kModeSlot : 0) |
           (decode_mode == 1 ? 1u << kModeRing : 0) | (sample_k > 0 ? 1u << kModeTopK : 0) |
           (nuc_on ? 1u << kModeNucleus : 0) | (lp_top >= 0 ? 1u << kModeLogprobs : 0) |
           (rules_on() ? 1u << kModeRules : 0) | (spec_max > 0 ? 1u << kModeSpec : 0);
}
// `turning_on` while the modes of the bit set `on` are on: LLMI_OK, or the first row's code with
// "<who>: <why>" as the error text
int Engine::refuse(const char* who, Mode turning_on, unsigned on) {
    for (const Refusal& r : kRefusals) {
        if (r.turning_on != turning_on || !(on >> r.on & 1)) continue;
        set_last_error(std::string("[llmi][ERROR] ") + who + ": " + r.why);
        return r.code;
    }
    return LLMI_OK;
}

// The legend of DecodeState::error (kernels.h), the one place it is written out.
std::string error_flag_text(int flags) {
    return std::to_string(flags) +
           " (1: token id out of range, 2: position overflow, 4: attention split count != device position, "
           "8: a tensor-parallel peer never arrived (one-shot exchange timeout), "
           "16: a prefill gate_up lo partial never arrived, 32: a ring-layer hand-off timed out, "
           "64: a fused q/k/v + attention wait timed out)";
}

int Engine::set_option(const std::string& name, int value) {
    if (name == "kpar") {
        LLMI_REQUIRE(value == 0 || value == 1, "set_option kpar: 1 on (default), 0 off");
        kpar_off = value == 0;
    } else if (name == "qkv_attn") {
        LLMI_REQUIRE(value == 0 || value == 1, "set_option qkv_attn: 1 one q/k/v + attention launch, 0 two");
        qa_fuse = value == 1;
    } else if (name == "qa_grid") {
        LLMI_REQUIRE(value >= 0, "set_option qa_grid: workgroups of the fused launch's GEMV part (0 = all resident)");
        qkv_attn_set_grid(value);
    } else if (name == "qa_o") {
        qa_o = value != 0;
    } else if (name == "qa_order") {
        qkv_attn_set_order(value);
    } else if (name == "qa_poll") {
        qkv_attn_set_poll(value);
    } else {
        LLMI_REQUIRE(false, "set_option: unknown option (kpar, qkv_attn, qa_o, qa_grid, qa_order, qa_poll)");
    }
    return invalidate();
}

int Engine::set_sampling(int k, uint64_t sd) {
    LLMI_REQUIRE(k >= 0 && k <= 16, "set_sampling: k must be in [0, 16] (0 = greedy)");
    if (k > 0) LLMI_TRY(refuse("set_sampling", kModeTopK));
    if (k > 0 && !samp_ids) {
        LLMI_HIP(hipMalloc(&samp_ids, 16 * sizeof(int32_t)));
        LLMI_HIP(hipMalloc(&samp_vals, 16 * sizeof(float)));
    }
    LLMI_TRY(invalidate());
    sample_k = k;
    sample_seed = sd;
    nuc_on = false;  // each of the two setters replaces the other
    return LLMI_OK;
}
int Engine::set_sampling_params(const llmi_sampling_params& p) {
    LLMI_TRY(refuse("set_sampling_params", kModeNucleus));
    LLMI_TRY(engine_nucleus_check(c.vocab, p.repetition_penalty, p.temperature, p.top_k, p.top_p));
    LLMI_TRY(invalidate());
    nuc = p;
    nuc_on = true;
    sample_k = 0;
    return LLMI_OK;
}

// -1 off, 0 the chosen token's logprob, 1..8 also that many alternatives. Independent of
// the sampler (it reads the raw row and whatever id the partials name).
int Engine::set_logprobs(int n_top) {
    LLMI_REQUIRE(n_top >= -1 && n_top <= kLpMaxTop, "set_logprobs: n_top must be -1 (off) or in [0, 8]");
    if (n_top >= 0) {
        LLMI_TRY(refuse("set_logprobs", kModeLogprobs));
        LLMI_TRY(engine_logprob_check(c.vocab, n_top));
    }
    LLMI_TRY(invalidate());
    if (n_top >= 0 && !lp_buf) LLMI_HIP(hipMalloc(&lp_buf, lp_bytes()));
    if (n_top >= 0 && n_top != lp_stride) {  // the record stride changes: nothing computed so far is readable
        LLMI_HIP(hipMemsetAsync(lp_buf, 0xFF, lp_bytes(), stream));
        LLMI_HIP(hipStreamSynchronize(stream));
        lp_stride = n_top;
    }
    lp_top = n_top;
    return LLMI_OK;
}
// records 0 .. n_valid - 1 (n_valid = positions stepped + 1; record 0 is never computed)
int Engine::logprobs_out(float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid, int* n_top) {
    LLMI_REQUIRE(lp_top >= 0 && lp_buf, "logprobs: set_logprobs first");
    LLMI_REQUIRE(n >= 0, "logprobs: n must be >= 0");
    LLMI_HIP(hipStreamSynchronize(stream));
    const int valid = prompt_len > 0 ? std::min(host_next_pos, c.max_seq) + 1 : 0;
    const size_t m = (size_t)std::min(n, valid);
    if (m > 0 && tok_lp) LLMI_HIP(hipMemcpy(tok_lp, lp_tok(), m * 4, hipMemcpyDeviceToHost));
    if (m > 0 && lp_top > 0 && top_ids) LLMI_HIP(hipMemcpy(top_ids, lp_ids(), m * lp_top * 4, hipMemcpyDeviceToHost));
    if (m > 0 && lp_top > 0 && top_lp) LLMI_HIP(hipMemcpy(top_lp, lp_tlp(), m * lp_top * 4, hipMemcpyDeviceToHost));
    if (n_valid) *n_valid = valid;
    if (n_top) *n_top = lp_top;
    return LLMI_OK;
}

// ------------------------------------------------------------ logit rules
// Rules are on while a bias, a non-zero penalty or an allowed set is present. The host logic
// that reads the caller's arrays is rules_host.h (checked under sanitizers on the CPU); here
// its results go to the engine's own device buffers with stream-ordered copies that have
// completed before the call returns, so no caller pointer and no host vector outlives it.
// A refused call has changed nothing.
//
// the rules launch enters the step, or its arguments change: the processed row's buffer
// exists from here on, and the captured steps are dropped
int Engine::rules_turn_on() {
    if (!lr_out) {
        LLMI_HIP(hipMalloc(&lr_out, (size_t)c.vocab * 4));
        LLMI_HIP(hipMemsetAsync(lr_out, 0, (size_t)c.vocab * 4, stream));
    }
    return invalidate();
}
int Engine::set_logit_rules(const int32_t* bias_ids, const float* bias_values, int n_bias, float presence,
                            float frequency, int count_prompt) {
    namespace rh = rules_host;
    LLMI_REQUIRE(rh::penalty_ok(presence) && rh::penalty_ok(frequency), "set_logit_rules: the penalties must be finite");
    LLMI_REQUIRE(count_prompt == 0 || count_prompt == 1, "set_logit_rules: count_prompt must be 0 or 1");
    std::vector<float> dense;
    const int st_ = rh::bias_to_dense(bias_ids, bias_values, n_bias, c.vocab, &dense);
    LLMI_REQUIRE(st_ == rh::kOk, std::string("set_logit_rules: ") + rh::message(st_));
    const bool pen = presence != 0.f || frequency != 0.f;
    if (n_bias > 0 || pen) {
        LLMI_TRY(refuse("set_logit_rules", kModeRules));
        LLMI_TRY(engine_logit_rules_check(c.vocab, c.max_seq, presence, frequency));
    }
    if (n_bias == 0 && !pen && !rules_on()) return LLMI_OK;  // off stays off: nothing to record
    if (n_bias > 0 && !lr_bias) LLMI_HIP(hipMalloc(&lr_bias, (size_t)c.vocab * 4));
    LLMI_TRY(rules_turn_on());  // (drops the captured steps: the launch arguments change)
    if (n_bias > 0) {
        LLMI_HIP(hipMemcpyAsync(lr_bias, dense.data(), (size_t)c.vocab * 4, hipMemcpyHostToDevice, stream));
        LLMI_HIP(hipStreamSynchronize(stream));  // dense is read until here
    }
    lr_bias_on = n_bias > 0;
    lr_presence = presence;
    lr_frequency = frequency;
    lr_count_prompt = count_prompt;
    return LLMI_OK;
}
// n = 0 with null ids removes the mask. Replacing the contents of a mask that is present leaves
// the captured steps as they are: the bitmap's address is fixed and the copy is stream-ordered.
int Engine::set_allowed(const int32_t* ids, int n) {
    namespace rh = rules_host;
    LLMI_REQUIRE(n >= 0, "set_allowed: n must be >= 0");
    LLMI_REQUIRE(n > 0 || !ids, "set_allowed: an empty allowed set (null ids with n = 0 removes the mask)");
    const bool was_on = rules_on();
    if (n == 0) {
        if (!lr_mask_on) return LLMI_OK;
        LLMI_HIP(hipMemsetAsync(lr_allowed, 0xFF, lr_words() * 4, stream));
        lr_mask_on = false;
        return rules_on() ? LLMI_OK : invalidate();  // the rules launch leaves the captured steps
    }
    std::vector<uint32_t> words;
    const int st_ = rh::ids_to_bitmap(ids, n, c.vocab, &words);
    LLMI_REQUIRE(st_ == rh::kOk, std::string("set_allowed: ") + rh::message(st_));
    if (!was_on) {
        LLMI_TRY(refuse("set_allowed", kModeRules));
        LLMI_TRY(engine_logit_rules_check(c.vocab, c.max_seq, 0.f, 0.f));
        LLMI_TRY(rules_turn_on());
    }
    LLMI_HIP(hipMemcpyAsync(lr_allowed, words.data(), words.size() * 4, hipMemcpyHostToDevice, stream));
    LLMI_HIP(hipStreamSynchronize(stream));  // words is read until here
    lr_mask_on = true;
    return LLMI_OK;
}
int Engine::clear_logit_rules() {
    if (!rules_on()) return LLMI_OK;
    LLMI_TRY(invalidate());
    if (lr_mask_on) {
        LLMI_HIP(hipMemsetAsync(lr_allowed, 0xFF, lr_words() * 4, stream));
        LLMI_HIP(hipStreamSynchronize(stream));
    }
    lr_bias_on = lr_mask_on = false;
    lr_presence = lr_frequency = 0.f;
    lr_count_prompt = 0;
    return LLMI_OK;
}
// the processed row of the last step (what the sampler, or the argmax, chose from)
int Engine::processed_out(float* out, int n) {
    LLMI_REQUIRE(out, "processed_logits: null out");
    LLMI_REQUIRE(n == c.vocab, "processed_logits: n must be the vocabulary size");
    LLMI_REQUIRE(rules_on() && lr_out, "processed_logits: the logit rules are off");
    LLMI_HIP(hipStreamSynchronize(stream));
    LLMI_HIP(hipMemcpy(out, lr_out, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

// ------------------------------------------------ persistent ring layer (mode 1)
bool Engine::ring_ok() const {
    // layers >= 2: a launch zeroes the NEXT launch's counter block ((l + 1) % L), which for
    // one layer would be its own, while its workgroups arrive on it
    return wdt == LLMI_F16 && edt == LLMI_F16 && c.tp_world == 1 && !grouped && c.layers >= 2 &&
           ring_supported(c.hidden, hl, c.head_dim, il, ql + 2 * kvrows, n_cu);
}
int Engine::set_decode_mode(int mode) {
    LLMI_REQUIRE(mode == 0 || mode == 1, "set_decode_mode: mode must be 0 (launches) or 1 (ring layer)");
    if (mode == 1) {
        LLMI_TRY(refuse("set_decode_mode", kModeRing));
        if (n_cu == 0) LLMI_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        if (!ring_ok()) {
            set_last_error("[llmi][ERROR] set_decode_mode: the ring layer needs fp16 weights, hidden 4096, "
                           "head_dim 128, heads dividing the CU count, tp_world 1, >= 2 layers");
            return LLMI_EUNSUPPORTED;
        }
        int per_cu = 0;
        LLMI_TRY(ring_residency(&per_cu));
        LLMI_REQUIRE(per_cu >= 1, "set_decode_mode: the ring layer's workgroup does not fit a CU");
        if (!rl_acc) {
            LLMI_HIP(hipMalloc(&rl_acc, (size_t)5 * c.hidden * 8));
            LLMI_HIP(hipMalloc(&rl_cnt, (size_t)c.layers * kRingCntWords * 4));
            LLMI_HIP(hipMalloc(&wdt_blob, (size_t)c.layers * il * c.hidden * 2));
        }
        LLMI_HIP(hipStreamSynchronize(stream));  // an eager ring step may still use what is zeroed here
        LLMI_HIP(hipMemset(rl_acc, 0, (size_t)5 * c.hidden * 8));
        LLMI_HIP(hipMemset(rl_cnt, 0, (size_t)c.layers * kRingCntWords * 4));
    }
    LLMI_TRY(invalidate());
    decode_mode = mode;
    return LLMI_OK;
}
int Engine::prepare_ring() {  // W_down^T of every layer, from the current weights
    if (wdt_valid) return LLMI_OK;
    for (int l = 0; l < c.layers; ++l) LLMI_TRY(transpose_f16_launch(layers[l].down, wdt_of(l), c.hidden, il, stream));
    LLMI_HIP(hipStreamSynchronize(stream));
    wdt_valid = true;
    return LLMI_OK;
}
// ring launch of layer l; wrap: the timing loop's cyclic form (every launch has a
// q/k/v phase and prepares layer (l + 1) % L's state)
RingArgs Engine::ring_args(int l, bool wrap) const {
    const int L = c.layers;
    const bool next = l + 1 < L || wrap;
    const Layer& Lw = layers[l];
    RingArgs r;
    r.w_o = Lw.o; r.w_gu = Lw.gu; r.w_dt = wdt_of(l); r.g_ffn = Lw.ffn_norm;
    if (next) {
        r.w_qkv = layers[(l + 1) % L].qkv;
        r.g_attn = layers[(l + 1) % L].attn_norm;
        r.qkv_out = qkv_buf;
    }
    r.attn_ws = attn_ws;
    r.acc_x = acc_a(l); r.acc_mid = acc_b(l); r.acc_out = acc_a(l + 1);
    r.zero0 = next ? acc_b(l + 1) : nullptr;
    r.zero1 = (l + 2 <= L || wrap) ? acc_a(l + 2) : nullptr;
    r.cnt = rl_cnt + (size_t)l * kRingCntWords;
    r.cnt_zero = rl_cnt + (size_t)((l + 1) % L) * kRingCntWords;
    r.hidden = c.hidden; r.heads = hl; r.inter = il; r.n_qkv = ql + 2 * kvrows; r.max_seq = c.max_seq;
    r.nact = rec_nact; r.eps = c.rms_eps; r.err = &st->error;
    r.stamps = stamp_ptr();
    return r;
}
int Engine::record_step_ring() {
    dbg_slot = 0;
    // step_start: x_0 into slot A0, zero A1 + B0 (adjacent) for layer 0's sums
    LLMI_TRY(step_start_launch(st, prompt, partials, lm_grid, tokens, embed, edt, c.hidden, x, acc_a(0), c.max_seq,
                               reinterpret_cast<unsigned*>(acc_a(1)), 4 * c.hidden, stream));
    GemvArgs q = qkv_args(0);
    q.x_fixed = acc_a(0);
    LLMI_TRY(gemv_launch(q, stream));
    for (int l = 0; l < c.layers; ++l) {
        AttnArgs at = attn_args(l);
        at.xacc = nullptr;  // the ring seeds the o_proj sum itself
        LLMI_TRY(attn_decode_launch(at, stream));
        LLMI_TRY(ring_layer_launch(ring_args(l), n_cu, stream));
    }
    GemvArgs h = lm_args();
    h.x_fixed = acc_a(c.layers);
    LLMI_TRY(gemv_launch(h, stream));
    return rec_sample();
}

int Engine::record_step() {
    LLMI_REQUIRE(!grouped, "engine: a group rank is stepped by its group");
    if (decode_mode == 1) return record_step_ring();
    dbg_slot = 0;
    LLMI_TRY(rec_start());
    for (int l = 0; l < c.layers; ++l) {
        LLMI_TRY(rec_attn(l));
        LLMI_TRY(exchange(xacc, c.hidden, 0));  // exact int64 sum of the fixed-point residual partials
        LLMI_TRY(rec_ffn(l));
        LLMI_TRY(exchange(res[(l + 1) % 2], c.hidden, 0));  // layer output (rank 0 carried the residual)
    }
    LLMI_TRY(rec_head());
    return exchange(partials, lm_grid, 2);  // max of the vocab-parallel argmax keys
}

int Engine::build_graph(int nact, hipGraphExec_t* exec) {
    rec_nact = nact;
    return graphs.get(nact, stream, [&]() { return record_step(); }, exec);
}

// ------------------------------------------------------------- driving
int Engine::set_prompt(const int32_t* ids, int n) {
    LLMI_REQUIRE(ids && n >= 1 && n <= c.max_seq, "set_prompt: need 1 <= n <= max_seq ids");
    for (int i = 0; i < n; ++i)
        LLMI_REQUIRE(ids[i] >= 0 && ids[i] < c.vocab, "set_prompt: token id out of range");
    DecodeState h{};
    h.next_pos = 0;
    h.cur_pos = 0;
    h.prompt_len = n;
    h.vocab = c.vocab;
    h.error = 0;
    LLMI_HIP(hipMemcpyAsync(prompt, ids, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    // (the epoch and what follows it are left alone: the fused q/k/v launch's granule tags
    // must never repeat the tag its buffer already holds, across prompts too)
    LLMI_HIP(hipMemcpyAsync(st, &h, offsetof(DecodeState, epoch), hipMemcpyHostToDevice, stream));
    if (lp_buf) LLMI_HIP(hipMemsetAsync(lp_buf, 0xFF, lp_bytes(), stream));  // NaN / id -1: not computed
    LLMI_HIP(hipStreamSynchronize(stream));
    host_next_pos = 0;
    prompt_len = n;
    sc_m = 0;  // the logits slab holds no row of this prompt
    return LLMI_OK;
}

int Engine::decode(int n, int use_graph) {
    LLMI_REQUIRE(prompt_len > 0, "decode: set_prompt first");
    LLMI_REQUIRE(c.tp_world == 1 || comm || xchg_mode >= 1 || xchg_loop,
                 "decode: tp_world > 1 needs an RCCL id at create or the one-shot exchange (xchg_open + set_exchange)");
    LLMI_REQUIRE(n >= 0 && host_next_pos + n <= c.max_seq, "decode: would run past max_seq");
    if (decode_mode == 1 && n > 0) LLMI_TRY(prepare_ring());
    const int k0 = nact_of(host_next_pos);
    std::vector<hipGraphExec_t> steps;  // every graph this run replays, captured before the first launch
    if (use_graph && n > 0) {
        steps.resize(nact_of(host_next_pos + n - 1) - k0 + 1);
        for (size_t j = 0; j < steps.size(); ++j) LLMI_TRY(build_graph(k0 + (int)j, &steps[j]));
    }
    for (int i = 0; i < n; ++i) {
        const int k = nact_of(host_next_pos + i);
        if (use_graph) {
            LLMI_HIP(hipGraphLaunch(steps[k - k0], stream));
        } else {
            rec_nact = k;
            LLMI_TRY(record_step());
        }
    }
    host_next_pos += n;
    return LLMI_OK;
}

int Engine::tokens_out(int32_t* out, int n, int* n_valid) {
    int valid = host_next_pos;
    if (host_next_pos >= prompt_len && host_next_pos <= c.max_seq) {
        LLMI_TRY(finalize_launch(st, partials, lm_grid, tokens, c.max_seq, stream));
        valid = host_next_pos + 1;
    }
    LLMI_HIP(hipStreamSynchronize(stream));
    DecodeState h;
    LLMI_HIP(hipMemcpy(&h, st, sizeof(h), hipMemcpyDeviceToHost));
    LLMI_REQUIRE(h.error == 0, "decode: device error flag " + error_flag_text(h.error));
    const int m = n < valid ? n : valid;
    if (m > 0) LLMI_HIP(hipMemcpy(out, tokens, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (n_valid) *n_valid = valid;
    return LLMI_OK;
}

}  // namespace llmi
