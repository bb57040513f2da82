// struct Batch: batched decode over sequence slots (engine.h).
#include "engine.h"

namespace llmi {

Batch::~Batch() {
    (void)graphs.drop(stream);  // before the slots whose launches they hold, and the stream
    while (r.size() > 1) r.pop_back();  // the borrowers before the lender
    r.clear();
    if (stream) (void)hipStreamDestroy(stream);
}

int Batch::init(const llmi_config& cfg, int n_seq, int dev) {
    LLMI_REQUIRE(n_seq >= 1 && n_seq <= kGemvRowsMax, "batch: n_seq must be 1..8");
    LLMI_TRY(Engine::refuse("batch", kModeSlot, Engine::config_modes(cfg)));
    LLMI_HIP(hipSetDevice(dev));
    LLMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (int i = 0; i < n_seq; ++i) {
        r.emplace_back(new Engine());
        r.back()->owner_graphs = &graphs;  // a slot's setters drop the batch's captured steps
        LLMI_TRY(r.back()->init(cfg, dev, nullptr, stream, i ? r[0].get() : nullptr, false));
        if (i) r.back()->pf_from = r[0].get();  // one prefill scratch per batch, slot 0's
    }
    return LLMI_OK;
}
int Batch::slot_ok(int seq) const {
    LLMI_REQUIRE(seq >= 0 && seq < (int)r.size(), "batch: seq out of range");
    return LLMI_OK;
}
int Batch::loaded() {  // slot 0 holds the weights every slot reads
    for (size_t i = 1; i < r.size(); ++i) r[i]->seed = r[0]->seed;
    for (auto& e : r) e->pfx_group = e->pfx_rows = 0;
    return graphs.drop(stream);
}
int Batch::reset(int seq) {
    LLMI_TRY(slot_ok(seq));
    LLMI_HIP(hipStreamSynchronize(stream));
    r[seq]->prompt_len = 0;
    r[seq]->host_next_pos = 0;
    r[seq]->pfx_group = r[seq]->pfx_rows = 0;
    return LLMI_OK;
}
int Batch::set_option(const std::string& name, int value) {
    LLMI_REQUIRE(name == "rows_mfma" || name == "gqa_attn" || name == "batch_attn" || name == "prefix_attn",
                 "batch set_option: unknown option (rows_mfma, gqa_attn, batch_attn, prefix_attn)");
    if (name == "prefix_attn") {  // record_step: forked slots read their shared leading rows once
        LLMI_REQUIRE(value == 0 || value == 1,
                     "batch set_option prefix_attn: 1 the slots of a fork group read the cache rows they share once per "
                     "step (one attention and one o_proj launch per layer), 0 off (default)");
        prefix_attn = value == 1;
        return graphs.drop(stream);
    }
    if (name == "batch_attn") {  // record_step: the slots' attention and o_proj as two launches a layer
        LLMI_REQUIRE(value == 0 || value == 1,
                     "batch set_option batch_attn: 1 one attention and one o_proj launch per layer for all active "
                     "slots, 0 one pair per slot (default)");
        batch_attn = value == 1;
        return graphs.drop(stream);
    }
    if (name == "gqa_attn") {  // every slot's per-sequence attention launch (Engine::gqa_attn)
        LLMI_REQUIRE(value == 0 || value == 1,
                     "batch set_option gqa_attn: 1 grouped-query decode attention on the matrix cores, 0 off (default)");
        for (auto& e : r) e->gqa_attn = value == 1;
        return graphs.drop(stream);
    }
    LLMI_REQUIRE(value == 0 || value == 1,
                 "batch set_option rows_mfma: 1 q/k/v, gate_up and down on the matrix cores, 0 off (default)");
    rows_mfma = value != 0;
    return graphs.drop(stream);  // the captured steps hold the other kernels
}
std::vector<int> Batch::active() const {
    std::vector<int> a;
    for (int i = 0; i < (int)r.size(); ++i)
        if (r[i]->prompt_len > 0) a.push_back(i);
    return a;
}

AttnPrefixArgs Batch::prefix_args(const std::vector<int>& act, int l) {
    AttnPrefixArgs p;
    for (int s : act) {
        p.group[p.b.n] = r[s]->pfx_group;
        p.rows[p.b.n] = r[s]->pfx_rows;
        attn_batch_add(p.b, r[s]->attn_args(l));
    }
    return p;
}

// one step of the active slots; every slot's rec_nact is set
int Batch::record_step(const std::vector<int>& act) {
    std::vector<Engine*> es;
    for (int s : act) es.push_back(r[s].get());
    // one multi-row GEMV from the active slots' own single-row arguments
    auto rows = [&](auto&& args_of) { return gemv_rows_of(es, stream, args_of); };
    for (Engine* e : es) LLMI_TRY(e->rec_start());
    const int L = r[0]->c.layers;
    if (es.size() == 1 && !rows_mfma) {  // one sequence: the engine's own single-row launches
        Engine& e = *es[0];
        for (int l = 0; l < L; ++l) {
            LLMI_TRY(e.rec_attn(l));
            LLMI_TRY(e.rec_ffn(l));
        }
        return e.rec_head();
    }
    // option rows_mfma: the three projections on the matrix cores where the kernel serves them
    // (debug stamps cleared as gemv_rows_of does), else the multi-row GEMV -- one slot: the
    // single-row GEMV with the engine's own arguments, stamps and all; the `tiny` preset of the
    // tests is served everywhere, so no test reaches either fallback
    auto proj = [&](auto&& args_of) {
        if (!rows_mfma) return rows(args_of);
        GemvRowsArgs p;
        for (Engine* e : es) gemv_rows_add(p, args_of(*e));
        p.a.stamps = nullptr;
        if (gemv_rows_mfma_supported(p)) return gemv_rows_mfma_launch(p, stream);
        return p.m == 1 ? gemv_launch(args_of(*es[0]), stream) : rows(args_of);
    };
    // option batch_attn, two or more slots: ONE attention launch and ONE o_proj launch for all of
    // them (attn_batch.hip), from each slot's own single-sequence arguments. With gqa_attn on as
    // well the attention stays per slot on the grouped-query kernel where it serves the shape
    // (the same workspace format) and only the o_proj is batched.
    auto attn_batched = [&](int l) -> int {
        AttnBatchArgs ab;
        OprojBatchArgs ob;
        for (Engine* e : es) {
            AttnArgs at = e->attn_args(l);
            at.gqa = e->gqa_attn;
            if (at.gqa && attn_gqa_supported(at)) LLMI_TRY(attn_decode_launch(at, stream));
            else attn_batch_add(ab, at);
            oproj_batch_add(ob, e->o_args(l));
        }
        ab.a.stamps = ob.a.stamps = nullptr;  // (debug stamps: a single-sequence form)
        if (ab.n) LLMI_TRY(attn_batch_launch(ab, stream));
        return oproj_batch_launch(ob, stream);
    };
    // option prefix_attn, two or more slots: attn_batched's structure with the attention launch
    // of attn_prefix.hip -- the members of a served fork group read their shared rows once; a
    // slot in no served group is a slot of attn_batch.hip inside the same launch, or, with
    // gqa_attn on, its own grouped-query launch as above.
    auto attn_prefixed = [&](int l) -> int {
        AttnPrefixArgs all = prefix_args(act, l), pa;
        const AttnPrefixPlan pl = attn_prefix_plan(all);
        OprojBatchArgs ob;
        for (size_t i = 0; i < es.size(); ++i) {
            AttnArgs at = es[i]->attn_args(l);
            at.gqa = es[i]->gqa_attn;
            if (pl.skip[i] == 0 && at.gqa && attn_gqa_supported(at)) {
                LLMI_TRY(attn_decode_launch(at, stream));
            } else {
                pa.group[pa.b.n] = all.group[i];
                pa.rows[pa.b.n] = all.rows[i];
                attn_batch_add(pa.b, at);
            }
            oproj_batch_add(ob, es[i]->o_args(l));
        }
        pa.b.a.stamps = ob.a.stamps = nullptr;  // (debug stamps: a single-sequence form)
        if (pa.b.n) LLMI_TRY(attn_prefix_launch(pa, stream));
        return oproj_batch_launch(ob, stream);
    };
    for (int l = 0; l < L; ++l) {
        LLMI_TRY(proj([&](Engine& e) { return e.qkv_args(l); }));
        if (prefix_attn && es.size() >= 2) {
            LLMI_TRY(attn_prefixed(l));
        } else if (batch_attn && es.size() >= 2) {
            LLMI_TRY(attn_batched(l));
        } else {
            for (Engine* e : es) {
                AttnArgs at = e->attn_args(l);
                at.gqa = e->gqa_attn;
                LLMI_TRY(e->rec_oproj(LLMI_OK, e->o_args(l), &at));
            }
        }
        LLMI_TRY(proj([&](Engine& e) { return e.gu_args(l); }));
        LLMI_TRY(proj([&](Engine& e) { return e.down_args(l); }));
    }
    if (es.size() == 1) return es[0]->rec_head();  // (option on: one slot takes the same projections)
    LLMI_TRY(rows([&](Engine& e) { return e.lm_args(); }));
    for (Engine* e : es) LLMI_TRY(e->rec_sample());
    return LLMI_OK;
}

int Batch::decode(int n, int use_graph) {
    const std::vector<int> act = active();
    LLMI_REQUIRE(!act.empty(), "batch decode: no active slot (set_prompt first)");
    LLMI_REQUIRE(n >= 0, "batch decode: n_steps must be >= 0");
    for (int s : act)
        LLMI_REQUIRE(r[s]->host_next_pos + n <= r[s]->c.max_seq, "batch decode: a slot would run past max_seq");
    for (int i = 0; i < n; ++i) {
        std::vector<int> key;  // (what a setter changes is not part of it: the setter drops the cache)
        for (int s : act) {
            r[s]->rec_nact = Engine::nact_of(r[s]->host_next_pos + i);
            key.push_back(s);
            key.push_back(r[s]->rec_nact);
        }
        // option prefix_attn: the plan is part of the step and a fork changes it without dropping
        // the captured steps, so every slot's (leader, P / 64) is part of the key
        if (prefix_attn && act.size() >= 2) {
            const AttnPrefixPlan pl = attn_prefix_plan(prefix_args(act, 0));
            for (size_t k = 0; k < act.size(); ++k) {
                key.push_back(act[pl.leader[k]]);
                key.push_back(pl.skip[k]);
            }
        }
        if (!use_graph) {
            LLMI_TRY(record_step(act));
            continue;
        }
        hipGraphExec_t step = nullptr;
        LLMI_TRY(graphs.get(key, stream, [&]() { return record_step(act); }, &step));
        LLMI_HIP(hipGraphLaunch(step, stream));
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
