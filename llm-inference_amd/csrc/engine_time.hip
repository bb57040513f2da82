// llmi_engine_time_kernel: one decode launch timed alone, cycling the layers.
#include "engine.h"

using llmi::Engine;

namespace {
// the timing run's events and captured graph: released on every return path
struct Timing {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipGraph_t cg = nullptr;
    hipGraphExec_t ce = nullptr;
    void release() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (ce) (void)hipGraphExecDestroy(ce);
        if (cg) (void)hipGraphDestroy(cg);
        t0 = t1 = nullptr;
        ce = nullptr;
        cg = nullptr;
    }
    ~Timing() { release(); }
};
}  // namespace

extern "C" {

int llmi_engine_time_kernel(llmi_engine* e, int which, int iters, float* avg_us, uint64_t* bytes) {
    LLMI_REQUIRE(e && avg_us && iters > 0, "time_kernel: bad arguments");
    Engine& g = e->e;
    LLMI_HIP(hipSetDevice(g.device));
    LLMI_REQUIRE(g.prompt_len > 0 && g.host_next_pos > 0, "time_kernel: decode at least one step first");
    g.rec_nact = Engine::nact_of(g.host_next_pos - 1);  // attention sized for the current position
    const size_t H = g.c.hidden;
    uint64_t b = 0;
    // launch i uses layer i % layers: every launch streams weights (and KV) the
    // previous launches did not touch, as in the decode loop -- replaying one layer
    // would serve its weights from the 256 MiB Infinity Cache and read high
    int li = 0;
    auto launch = [&]() -> int {
        const int l = li++ % g.c.layers;
        switch (which) {
            case 0: return llmi::gemv_launch(g.qkv_args(l), g.stream);
            case 1: return llmi::attn_decode_launch(g.attn_args(l), g.stream);
            case 2: return llmi::attn_oproj_launch(g.o_args(l), g.stream);
            case 3: return llmi::gemv_launch(g.gu_args(l), g.stream);
            case 4: return llmi::gemv_launch(g.down_args(l), g.stream);
            case 5: return llmi::gemv_launch(g.lm_args(), g.stream);
            case 6:
            case 7: {  // the per-token TP exchange: one residual all-reduce (int64, hidden)
                ncclResult_t r = ncclAllReduce(g.xacc, g.xacc, H, ncclInt64, ncclSum, g.comm, g.stream);
                LLMI_REQUIRE(r == ncclSuccess, std::string("ncclAllReduce(int64): ") + ncclGetErrorString(r));
                return LLMI_OK;
            }
            case 8:
            case 9:  // the same exchange over the one-shot peer path
                return llmi::xchg_launch(g.xchg_args(g.xacc, (int)H, 0, 3), g.stream);
            case 10:  // the persistent ring layer (o_proj, gate_up, down, next q/k/v)
                return llmi::ring_layer_launch(g.ring_args(l, true), g.n_cu, g.stream);
            case 11: {  // the fused q/k/v + attention launch (the decode default; consecutive launches
                        // cycle layers, so each finds the previous layer's tags in the granule buffer)
                llmi::GemvArgs q = g.qkv_args(l);
                llmi::AttnArgs at = g.attn_args(l);
                q.kpar = 0;
                g.tag_qkv(q, at, l);
                at.xacc = nullptr;  // (timing only: no residual seed)
                return llmi::qkv_attn_launch(q, at, g.stream);
            }
        }
        LLMI_REQUIRE(false, "time_kernel: which must be 0..11");
    };
    LLMI_REQUIRE(which < 6 || which > 7 || g.comm != nullptr,
                 "time_kernel: the all-reduce needs an RCCL communicator (tp_id)");
    LLMI_REQUIRE(which < 8 || which > 9 || g.peers_ready, "time_kernel: the one-shot exchange needs xchg_open");
    LLMI_REQUIRE(which != 10 || (g.decode_mode == 1 && g.wdt_valid), "time_kernel: the ring layer needs decode mode 1");
    // a [rows, cols] linear weight of dtype dt with its scales
    auto lin = [&](int dt, uint64_t rows, uint64_t cols) -> uint64_t {
        return Engine::lin_bytes(dt, rows, cols) + Engine::scale_bytes(dt, rows, cols);
    };
    auto qkv_bytes = [&]() -> uint64_t { return lin(g.wdt, g.ql + 2 * g.kvrows, H); };
    auto attn_bytes = [&](uint64_t* out) -> int {  // the K/V rows read up to the device's position, one row written
        llmi::DecodeState hs;
        LLMI_HIP(hipMemcpy(&hs, g.st, sizeof(hs), hipMemcpyDeviceToHost));
        // a row's bytes: its elements, and with the int8 cache its fp16 scale
        const uint64_t rb = (uint64_t)g.c.head_dim * llmi::dtype_size(g.c.kv_dtype) + (g.kscale ? 2 : 0);
        *out = (uint64_t)2 * (hs.cur_pos + 1) * g.kvl * rb + 2ull * g.kvl * rb;
        return LLMI_OK;
    };
    switch (which) {
        case 0: b = qkv_bytes(); break;
        case 1: LLMI_TRY(attn_bytes(&b)); break;
        case 2: b = lin(g.odt(), H, g.ql); break;
        case 3: b = lin(g.wdt, 2 * g.il, H); break;
        case 4: b = lin(g.wdt, H, g.il); break;
        case 5: b = (uint64_t)g.vl * H * g.esz; break;
        case 6:
        case 7:
        case 8:
        case 9: b = (uint64_t)H * 8; break;
        case 10:  // (fp16 only: no scales)
            b = lin(g.wdt, H, g.ql) + lin(g.wdt, 3ull * g.il, H) + lin(g.wdt, g.ql + 2 * g.kvrows, H);
            break;
        case 11:
            LLMI_TRY(attn_bytes(&b));
            b += qkv_bytes();
            break;
    }
    // timing launches modify the residual stream (o/down epilogues add into x),
    // so save and restore the small activation state around them
    std::vector<char> save(H * 4), save_fx(3 * H * 8);
    LLMI_HIP(hipMemcpyAsync(save.data(), g.x, H * 4, hipMemcpyDeviceToHost, g.stream));
    long long* fx[3] = {g.xacc, g.res[0], g.res[1]};
    for (int i = 0; i < 3; ++i)
        LLMI_HIP(hipMemcpyAsync(save_fx.data() + i * H * 8, fx[i], H * 8, hipMemcpyDeviceToHost, g.stream));
    // the attention launches write the current position's K/V row into every layer they
    // cycle through (from the last layer's q/k/v): keep each layer's row at cur_pos
    llmi::DecodeState hst{};
    std::vector<char> save_kv;
    std::vector<uint16_t> save_ks;
    const size_t kv_eb = llmi::dtype_size(g.c.kv_dtype), kv_row = (size_t)g.c.head_dim * kv_eb;
    const size_t kv_pitch = (size_t)g.c.max_seq * kv_row;
    auto kv_rows = [&](int l, int v) { return g.kv_layer(l, v) + (size_t)hst.cur_pos * kv_row; };
    LLMI_REQUIRE(which != 11 || (g.layers.size() >= 2 && g.c.layers < 128),
                 "time_kernel: the fused q/k/v + attention launch cycles >= 2 layers (its tags must change)");
    if (which == 1 || which == 11) {
        LLMI_HIP(hipMemcpyAsync(&hst, g.st, sizeof(hst), hipMemcpyDeviceToHost, g.stream));
        LLMI_HIP(hipStreamSynchronize(g.stream));
        save_kv.resize((size_t)g.c.layers * 2 * g.kvl * kv_row);
        if (g.kscale) {  // int8 cache: the rows' scales too
            save_ks.resize((size_t)g.c.layers * 2 * g.kvl);
            for (int l = 0; l < g.c.layers; ++l)
                for (int v = 0; v < 2; ++v)
                    LLMI_HIP(hipMemcpy2D(save_ks.data() + ((size_t)l * 2 + v) * g.kvl, 2, g.kv_scale_layer(l, v) + hst.cur_pos,
                                         (size_t)g.c.max_seq * 2, 2, g.kvl, hipMemcpyDeviceToHost));
        }
        for (int l = 0; l < g.c.layers; ++l)
            for (int v = 0; v < 2; ++v)
                LLMI_HIP(hipMemcpy2D(save_kv.data() + ((size_t)l * 2 + v) * g.kvl * kv_row, kv_row, kv_rows(l, v),
                                     kv_pitch, kv_row, g.kvl, hipMemcpyDeviceToHost));
    }
    std::vector<char> save_rl;
    if (which == 10) {
        save_rl.resize((size_t)5 * H * 8);
        LLMI_HIP(hipMemcpyAsync(save_rl.data(), g.rl_acc, save_rl.size(), hipMemcpyDeviceToHost, g.stream));
    }
    LLMI_TRY(launch());  // warm
    auto run = [&]() -> int {
        for (int i = 0; i < iters; ++i) LLMI_TRY(launch());
        return LLMI_OK;
    };
    Timing t;
    if (which == 7 || which == 9) {  // the exchanges captured into one graph, as the decode step replays them
        LLMI_TRY(llmi::capture(g.stream, run, &t.cg, &t.ce));
        LLMI_HIP(hipGraphLaunch(t.ce, g.stream));  // warm
    }
    LLMI_HIP(hipEventCreate(&t.t0));
    LLMI_HIP(hipEventCreate(&t.t1));
    LLMI_HIP(hipEventRecord(t.t0, g.stream));
    if (t.ce) {
        LLMI_HIP(hipGraphLaunch(t.ce, g.stream));
    } else {
        LLMI_TRY(run());
    }
    LLMI_HIP(hipEventRecord(t.t1, g.stream));
    LLMI_HIP(hipEventSynchronize(t.t1));
    float ms = 0.f;
    LLMI_HIP(hipEventElapsedTime(&ms, t.t0, t.t1));
    t.release();
    LLMI_HIP(hipMemcpy(g.x, save.data(), H * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < 3; ++i) LLMI_HIP(hipMemcpy(fx[i], save_fx.data() + i * H * 8, H * 8, hipMemcpyHostToDevice));
    if (which == 1 || which == 11)
        for (int l = 0; l < g.c.layers; ++l)
            for (int v = 0; v < 2; ++v)
                LLMI_HIP(hipMemcpy2D(kv_rows(l, v), kv_pitch, save_kv.data() + ((size_t)l * 2 + v) * g.kvl * kv_row,
                                     kv_row, kv_row, g.kvl, hipMemcpyHostToDevice));
    if ((which == 1 || which == 11) && g.kscale)
        for (int l = 0; l < g.c.layers; ++l)
            for (int v = 0; v < 2; ++v)
                LLMI_HIP(hipMemcpy2D(g.kv_scale_layer(l, v) + hst.cur_pos, (size_t)g.c.max_seq * 2,
                                     save_ks.data() + ((size_t)l * 2 + v) * g.kvl, 2, 2, g.kvl, hipMemcpyHostToDevice));
    if (which == 10) {  // accumulators back, every layer's counters zero again
        LLMI_HIP(hipMemcpy(g.rl_acc, save_rl.data(), save_rl.size(), hipMemcpyHostToDevice));
        LLMI_HIP(hipMemset(g.rl_cnt, 0, (size_t)g.c.layers * llmi::kRingCntWords * 4));
    }
    *avg_us = ms * 1000.f / iters;
    if (bytes) *bytes = b;
    return LLMI_OK;
}

}  // extern "C"
