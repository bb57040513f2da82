// struct Group: the in-process tensor-parallel group (engine.h).
#include "engine.h"

namespace llmi {

Group::~Group() {
    (void)graphs.drop(stream);  // before the ranks whose launches they hold, and the stream
    r.clear();
    if (ptrs) (void)hipFree(ptrs);
    if (stream) (void)hipStreamDestroy(stream);
}

int Group::init(const llmi_config& cfg, int world, int dev) {
    LLMI_REQUIRE(world >= 1 && world <= 64, "group: world must be 1..64");
    LLMI_TRY(Engine::refuse("group", kModeTp, Engine::config_modes(cfg)));
    LLMI_HIP(hipSetDevice(dev));
    LLMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (int i = 0; i < world; ++i) {
        llmi_config c = cfg;
        c.tp_rank = i;
        c.tp_world = world;
        r.emplace_back(new Engine());
        LLMI_TRY(r.back()->init(c, dev, nullptr, stream));
    }
    std::vector<void*> h(4 * world);
    for (int i = 0; i < world; ++i) {
        h[i] = r[i]->xacc;
        h[world + i] = r[i]->res[0];
        h[2 * world + i] = r[i]->res[1];
        h[3 * world + i] = r[i]->partials;
    }
    LLMI_HIP(hipMalloc(&ptrs, h.size() * sizeof(void*)));
    LLMI_HIP(hipMemcpy(ptrs, h.data(), h.size() * sizeof(void*), hipMemcpyHostToDevice));
    return LLMI_OK;
}

int Group::set_exchange(int mode) {
    LLMI_REQUIRE(mode >= 0 && mode <= 2,
                 "group set_exchange: mode must be 0 (reduce kernel), 1 (one-shot) or 2 (push fused into the producers)");
    if (mode >= 1) {
        std::vector<char*> inboxes;
        for (auto& e : r) {
            LLMI_TRY(e->alloc_xchg());
            inboxes.push_back(e->inbox);
        }
        for (auto& e : r) LLMI_TRY(e->set_peers(inboxes));  // same device: the inboxes themselves
    }
    LLMI_TRY(graphs.drop(stream));  // the captured steps change
    xchg_mode = mode;
    for (auto& e : r) e->tail_mode = mode == 2 ? 1 : 0;
    return LLMI_OK;
}
// slot: 0 xacc, 1 res[0], 2 res[1], 3 argmax partials
int Group::reduce(int slot, int n, int op) {
    const int W = (int)r.size();
    if (W == 1) return LLMI_OK;
    if (xchg_mode == 0) return group_reduce_launch(ptrs + slot * W, W, n, op, stream);
    auto buf = [&](Engine& e) -> void* {
        return slot == 0 ? (void*)e.xacc : slot == 3 ? (void*)e.partials : (void*)e.res[slot - 1];
    };
    if (xchg_mode == 1)  // (mode 2: the producers pushed already)
        for (auto& e : r) LLMI_TRY(xchg_launch(e->xchg_args(buf(*e), n, op, 1), stream));
    for (auto& e : r) LLMI_TRY(xchg_launch(e->xchg_args(buf(*e), n, op, 2), stream));
    return LLMI_OK;
}

int Group::record_step(int nact) {
    const int H = r[0]->c.hidden;
    for (auto& e : r) e->rec_nact = nact;
    for (auto& e : r) LLMI_TRY(e->rec_start());
    for (int l = 0; l < r[0]->c.layers; ++l) {
        for (auto& e : r) LLMI_TRY(e->rec_attn(l));
        LLMI_TRY(reduce(0, H, 0));
        for (auto& e : r) LLMI_TRY(e->rec_ffn(l));
        LLMI_TRY(reduce(1 + (l + 1) % 2, H, 0));
    }
    for (auto& e : r) LLMI_TRY(e->rec_head());
    return reduce(3, r[0]->lm_grid, 2);
}

int Group::decode(int n, int use_graph) {
    Engine& e0 = *r[0];
    LLMI_REQUIRE(e0.prompt_len > 0, "group decode: set_prompt first");
    LLMI_REQUIRE(n >= 0 && e0.host_next_pos + n <= e0.c.max_seq, "group decode: would run past max_seq");
    const int k0 = Engine::nact_of(e0.host_next_pos);
    std::vector<hipGraphExec_t> steps;  // every graph this run replays, captured before the first launch
    if (use_graph && n > 0) {
        steps.resize(Engine::nact_of(e0.host_next_pos + n - 1) - k0 + 1);
        for (int k = k0; k < k0 + (int)steps.size(); ++k)
            LLMI_TRY(graphs.get(k, stream, [&]() { return record_step(k); }, &steps[k - k0]));
    }
    for (int i = 0; i < n; ++i) {
        const int k = Engine::nact_of(e0.host_next_pos + i);
        if (use_graph)
            LLMI_HIP(hipGraphLaunch(steps[k - k0], stream));
        else
            LLMI_TRY(record_step(k));
    }
    for (auto& e : r) e->host_next_pos += n;
    return LLMI_OK;
}

}  // namespace llmi
