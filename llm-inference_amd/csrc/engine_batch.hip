// struct Batch: batched decode over sequence slots (engine.h).
#include "engine.h"

namespace llmi {

void Batch::clear_graphs() {
    for (auto& kv : graphs) {
        if (kv.second.second) (void)hipGraphExecDestroy(kv.second.second);
        if (kv.second.first) (void)hipGraphDestroy(kv.second.first);
    }
    graphs.clear();
}
Batch::~Batch() {
    clear_graphs();
    while (r.size() > 1) r.pop_back();  // the borrowers before the lender
    r.clear();
    if (stream) (void)hipStreamDestroy(stream);
}

int Batch::init(const llmi_config& cfg, int n_seq, int dev) {
    LLMI_REQUIRE(n_seq >= 1 && n_seq <= kGemvRowsMax, "batch: n_seq must be 1..8");
    if (cfg.tp_world != 1) {
        set_last_error("[llmi][ERROR] batch: tensor-parallel batches are not built (tp_world must be 1)");
        return LLMI_EUNSUPPORTED;
    }
    if (cfg.weight_dtype == LLMI_I4) {
        set_last_error("[llmi][ERROR] batch: int4 weights are not built into the multi-row GEMV (use an Engine)");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_HIP(hipSetDevice(dev));
    LLMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (int i = 0; i < n_seq; ++i) {
        r.emplace_back(new Engine());
        LLMI_TRY(r.back()->init(cfg, dev, nullptr, stream, i ? r[0].get() : nullptr, false));
        if (i) r.back()->pf_from = r[0].get();  // one prefill scratch per batch, slot 0's
    }
    return LLMI_OK;
}
int Batch::slot_ok(int seq) const {
    LLMI_REQUIRE(seq >= 0 && seq < (int)r.size(), "batch: seq out of range");
    return LLMI_OK;
}
int Batch::drop_graphs() {
    if (!graphs.empty()) {
        LLMI_HIP(hipStreamSynchronize(stream));  // a replay may still be in flight
        clear_graphs();
    }
    return LLMI_OK;
}
int Batch::loaded() {  // slot 0 holds the weights every slot reads
    for (size_t i = 1; i < r.size(); ++i) r[i]->seed = r[0]->seed;
    return drop_graphs();
}
int Batch::reset(int seq) {
    LLMI_TRY(slot_ok(seq));
    LLMI_HIP(hipStreamSynchronize(stream));
    r[seq]->prompt_len = 0;
    r[seq]->host_next_pos = 0;
    return LLMI_OK;
}
std::vector<int> Batch::active() const {
    std::vector<int> a;
    for (int i = 0; i < (int)r.size(); ++i)
        if (r[i]->prompt_len > 0) a.push_back(i);
    return a;
}

// one multi-row GEMV from the active slots' own single-row arguments
template <typename F>
int Batch::rows(const std::vector<int>& act, F&& args_of) {
    GemvRowsArgs p;
    p.m = (int)act.size();
    for (int i = 0; i < p.m; ++i) {
        const GemvArgs a = args_of(*r[act[i]]);
        if (i == 0) p.a = a;
        GemvRow& w = p.row[i];
        w.x = a.x; w.x_fixed = a.x_fixed; w.x_out = a.x_out; w.y = a.y; w.resid = a.resid;
        w.yacc = a.yacc; w.yacc_base = a.yacc_base; w.yacc_copy = a.yacc_copy; w.partials = a.partials;
        w.seed_src = a.seed_src; w.seed_dst = a.seed_dst;
    }
    return gemv_rows_launch(p, stream);
}

// one step of the active slots; every slot's rec_nact is set
int Batch::record_step(const std::vector<int>& act) {
    for (int s : act) LLMI_TRY(r[s]->rec_start());
    const int L = r[0]->c.layers;
    if (act.size() == 1) {  // one sequence: the engine's own single-row launches
        Engine& e = *r[act[0]];
        for (int l = 0; l < L; ++l) {
            LLMI_TRY(e.rec_attn(l));
            LLMI_TRY(e.rec_ffn(l));
        }
        return e.rec_head();
    }
    for (int l = 0; l < L; ++l) {
        LLMI_TRY(rows(act, [&](Engine& e) { return e.qkv_args(l); }));
        for (int s : act) {
            Engine& e = *r[s];
            const AttnArgs at = e.attn_args(l);
            LLMI_TRY(e.rec_oproj(LLMI_OK, e.o_args(l), &at));
        }
        LLMI_TRY(rows(act, [&](Engine& e) { return e.gu_args(l); }));
        LLMI_TRY(rows(act, [&](Engine& e) { return e.down_args(l); }));
    }
    LLMI_TRY(rows(act, [&](Engine& e) { return e.lm_args(); }));
    for (int s : act) LLMI_TRY(r[s]->rec_sample());
    return LLMI_OK;
}

int Batch::decode(int n, int use_graph) {
    const std::vector<int> act = active();
    LLMI_REQUIRE(!act.empty(), "batch decode: no active slot (set_prompt first)");
    LLMI_REQUIRE(n >= 0, "batch decode: n_steps must be >= 0");
    for (int s : act)
        LLMI_REQUIRE(r[s]->host_next_pos + n <= r[s]->c.max_seq, "batch decode: a slot would run past max_seq");
    for (int i = 0; i < n; ++i) {
        std::vector<int> key;
        for (int s : act) {
            r[s]->rec_nact = Engine::nact_of(r[s]->host_next_pos + i);
            key.push_back(s);
            key.push_back(r[s]->rec_nact);
            key.push_back(r[s]->lp_top);  // the slot's logprob launch (or none) is part of the step
        }
        if (!use_graph) {
            LLMI_TRY(record_step(act));
            continue;
        }
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            if (graphs.size() >= kMaxGraphs) LLMI_TRY(drop_graphs());
            hipGraph_t h = nullptr;
            hipGraphExec_t x = nullptr;
            LLMI_TRY(capture(stream, [&]() { return record_step(act); }, &h, &x));
            it = graphs.emplace(key, std::make_pair(h, x)).first;
        }
        LLMI_HIP(hipGraphLaunch(it->second.second, stream));
    }
    for (int s : act) r[s]->host_next_pos += n;
    return LLMI_OK;
}

// slot seq's prefill / scored prefill on the batch's stream, through slot 0's prefill scratch;
// the slot ends where n decode steps would have left it (host_next_pos: the next step's key)
int Batch::prefill(int seq, int n, int split, bool scored) {
    LLMI_TRY(slot_ok(seq));
    LLMI_REQUIRE(r[seq]->prompt_len > 0, "batch prefill: the slot is idle (set_prompt first)");
    return r[seq]->prefill(n, split, scored);
}

}  // namespace llmi
