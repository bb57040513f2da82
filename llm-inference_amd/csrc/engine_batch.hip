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
    return graphs.drop(stream);
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

// one step of the active slots; every slot's rec_nact is set
int Batch::record_step(const std::vector<int>& act) {
    std::vector<Engine*> es;
    for (int s : act) es.push_back(r[s].get());
    // one multi-row GEMV from the active slots' own single-row arguments
    auto rows = [&](auto&& args_of) { return gemv_rows_of(es, stream, args_of); };
    for (Engine* e : es) LLMI_TRY(e->rec_start());
    const int L = r[0]->c.layers;
    if (es.size() == 1) {  // one sequence: the engine's own single-row launches
        Engine& e = *es[0];
        for (int l = 0; l < L; ++l) {
            LLMI_TRY(e.rec_attn(l));
            LLMI_TRY(e.rec_ffn(l));
        }
        return e.rec_head();
    }
    for (int l = 0; l < L; ++l) {
        LLMI_TRY(rows([&](Engine& e) { return e.qkv_args(l); }));
        for (Engine* e : es) {
            const AttnArgs at = e->attn_args(l);
            LLMI_TRY(e->rec_oproj(LLMI_OK, e->o_args(l), &at));
        }
        LLMI_TRY(rows([&](Engine& e) { return e.gu_args(l); }));
        LLMI_TRY(rows([&](Engine& e) { return e.down_args(l); }));
    }
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
