// The C ABI of the engine, the in-process group and the batch (include/llmi.h), and the
// llmi_tp_* communicator calls. llmi_engine_time_kernel is in engine_time.hip.
#include "engine.h"

using llmi::Engine;

namespace {
float h2f(uint16_t h) {
    __half v;
    std::memcpy(&v, &h, 2);
    return __half2float(v);
}
}  // namespace

extern "C" {

int llmi_config_preset(const char* name, llmi_config* cfg) {
    LLMI_REQUIRE(name && cfg, "preset: null argument");
    llmi_config c{};
    c.hidden = 4096; c.heads = 32; c.kv_heads = 32; c.head_dim = 128; c.inter = 11008;
    c.layers = 32; c.vocab = 32000; c.max_seq = 2048; c.rms_eps = 1e-5f; c.rope_base = 10000.f;
    c.weight_dtype = LLMI_F16; c.kv_dtype = LLMI_F16; c.tp_rank = 0; c.tp_world = 1;
    const std::string n(name);
    if (n == "llama2-7b") {
    } else if (n == "llama2-13b") {
        c.hidden = 5120; c.heads = 40; c.kv_heads = 40; c.inter = 13824; c.layers = 40;
    } else if (n == "tiny") {
        c.hidden = 512; c.heads = 4; c.kv_heads = 4; c.inter = 1024; c.layers = 2; c.max_seq = 64;
    } else {
        LLMI_REQUIRE(false, "preset: unknown name " + n);
    }
    *cfg = c;
    return LLMI_OK;
}

int llmi_tp_unique_id(void* out128) {
    LLMI_REQUIRE(out128, "tp_unique_id: null");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    LLMI_REQUIRE(r == ncclSuccess, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    static_assert(sizeof(id) == 128, "ncclUniqueId must be 128 bytes");
    std::memcpy(out128, &id, sizeof(id));
    return LLMI_OK;
}

int llmi_tp_comm_create(const void* tp_id, int world, int rank, int device, llmi_tp_comm** out) {
    LLMI_REQUIRE(tp_id && out && world >= 1 && rank >= 0 && rank < world, "tp_comm_create: bad arguments");
    *out = nullptr;
    LLMI_HIP(hipSetDevice(device));
    ncclUniqueId id;
    std::memcpy(&id, tp_id, sizeof(id));
    auto h = std::make_unique<llmi_tp_comm>();
    ncclResult_t r = ncclCommInitRank(&h->c, world, id, rank);
    LLMI_REQUIRE(r == ncclSuccess, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    *out = h.release();
    return LLMI_OK;
}

int llmi_tp_allreduce(llmi_tp_comm* comm, void* buf, size_t count, int dtype, llmi_stream_t stream) {
    LLMI_REQUIRE(comm && comm->c && (buf || count == 0), "tp_allreduce: bad arguments");
    ncclDataType_t t;
    switch (dtype) {
        case LLMI_F32: t = ncclFloat32; break;
        case LLMI_F16: t = ncclFloat16; break;
        case LLMI_I32: t = ncclInt32; break;
        case LLMI_I64: t = ncclInt64; break;
        default: LLMI_REQUIRE(false, "tp_allreduce: dtype must be f32, f16, i32 or i64");
    }
    if (count == 0) return LLMI_OK;
    ncclResult_t r = ncclAllReduce(buf, buf, count, t, ncclSum, comm->c, reinterpret_cast<hipStream_t>(stream));
    LLMI_REQUIRE(r == ncclSuccess, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    return LLMI_OK;
}

int llmi_tp_comm_destroy(llmi_tp_comm* comm) {
    if (!comm) return LLMI_OK;
    ncclResult_t r = comm->c ? ncclCommDestroy(comm->c) : ncclSuccess;
    delete comm;
    LLMI_REQUIRE(r == ncclSuccess, std::string("ncclCommDestroy: ") + ncclGetErrorString(r));
    return LLMI_OK;
}

int llmi_engine_create(const llmi_config* cfg, int device, const void* tp_id, llmi_engine** out) {
    LLMI_REQUIRE(cfg && out, "engine_create: null argument");
    *out = nullptr;
    auto h = std::make_unique<llmi_engine>();
    int rc = h->e.init(*cfg, device, tp_id);
    if (rc != LLMI_OK) return rc;
    *out = h.release();
    return LLMI_OK;
}

int llmi_engine_destroy(llmi_engine* e) {
    if (e) {
        (void)hipSetDevice(e->e.device);
        (void)hipStreamSynchronize(e->e.stream);
        delete e;
    }
    return LLMI_OK;
}

int llmi_engine_load_synthetic(llmi_engine* e, uint64_t seed) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.load_synthetic(seed);
}

int llmi_engine_load_tensor(llmi_engine* e, const char* name, const float* host, size_t count) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.load_tensor(name, host, count);
}

int llmi_engine_load_tensor_quantized(llmi_engine* e, const char* name, const float* host, size_t count) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.load_tensor(name, host, count, true);
}

int llmi_engine_load_bin_quantized(llmi_engine* e, const char* weight_path) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.load_bin(weight_path, true);
}

int llmi_engine_set_sampling(llmi_engine* e, int k, uint64_t seed) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_sampling(k, seed);
}

int llmi_engine_set_sampling_params(llmi_engine* e, const llmi_sampling_params* p) {
    LLMI_REQUIRE(e && p, "engine_set_sampling_params: null engine or params");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_sampling_params(*p);
}

int llmi_engine_load_bin(llmi_engine* e, const char* weight_path) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.load_bin(weight_path);
}

int llmi_engine_set_logprobs(llmi_engine* e, int n_top) {
    LLMI_REQUIRE(e, "engine_set_logprobs: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_logprobs(n_top);
}

int llmi_engine_logprobs(llmi_engine* e, float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid,
                         int* n_top) {
    LLMI_REQUIRE(e, "engine_logprobs: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.logprobs_out(tok_lp, top_ids, top_lp, n, n_valid, n_top);
}

int llmi_engine_set_logit_rules(llmi_engine* e, const int32_t* bias_ids, const float* bias_values, int n_bias,
                                float presence_penalty, float frequency_penalty, int count_prompt) {
    LLMI_REQUIRE(e, "engine_set_logit_rules: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_logit_rules(bias_ids, bias_values, n_bias, presence_penalty, frequency_penalty, count_prompt);
}

int llmi_engine_set_allowed(llmi_engine* e, const int32_t* ids, int n) {
    LLMI_REQUIRE(e, "engine_set_allowed: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_allowed(ids, n);
}

int llmi_engine_clear_logit_rules(llmi_engine* e) {
    LLMI_REQUIRE(e, "engine_clear_logit_rules: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.clear_logit_rules();
}

int llmi_engine_processed_logits(llmi_engine* e, float* out, int n) {
    LLMI_REQUIRE(e, "engine_processed_logits: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.processed_out(out, n);
}

int llmi_engine_set_prompt(llmi_engine* e, const int32_t* ids, int n) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_prompt(ids, n);
}

int llmi_engine_decode(llmi_engine* e, int n_steps, int use_graph) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.decode(n_steps, use_graph);
}

int llmi_engine_set_speculation(llmi_engine* e, int max_draft) {
    LLMI_REQUIRE(e, "engine_set_speculation: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_speculation(max_draft);
}

int llmi_engine_verify(llmi_engine* e, const int32_t* draft, int n_draft, int use_graph, int* n_accepted) {
    LLMI_REQUIRE(e, "engine_verify: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.verify(draft, n_draft, use_graph, n_accepted);
}

int llmi_lookup_draft(const int32_t* ids, int n, int ngram_max, int ngram_min, int max_draft, int32_t* out,
                      int* n_out) {
    return llmi::lookup_draft(ids, n, ngram_max, ngram_min, max_draft, out, n_out);
}

int llmi_engine_generate_lookup(llmi_engine* e, int n_steps, int max_draft, int ngram_max, int ngram_min,
                                int use_graph, llmi_spec_stats* stats) {
    LLMI_REQUIRE(e, "engine_generate_lookup: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.generate_lookup(n_steps, max_draft, ngram_max, ngram_min, use_graph, stats);
}

int llmi_engine_generate_draft(llmi_engine* target, llmi_engine* draft, int n_steps, int max_draft,
                               int draft_prefill, int use_graph, llmi_spec_stats* stats) {
    LLMI_REQUIRE(target && draft, "engine_generate_draft: null engine");
    LLMI_HIP(hipSetDevice(target->e.device));
    return target->e.generate_draft(draft->e, n_steps, max_draft, draft_prefill, use_graph, stats);
}

int llmi_engine_edit(llmi_engine* e, int keep, const int32_t* ids, int n) {
    LLMI_REQUIRE(e, "engine_edit: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.edit(keep, ids, n);
}

int llmi_engine_position(llmi_engine* e, int* next_pos, int* prompt_len) {
    LLMI_REQUIRE(e, "engine_position: null engine");
    if (next_pos) *next_pos = e->e.host_next_pos;
    if (prompt_len) *prompt_len = e->e.prompt_len;
    return LLMI_OK;
}

int llmi_engine_prefill(llmi_engine* e, int n_tokens, int exact) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_REQUIRE(exact >= 0 && exact <= 2, "prefill: exact must be 0 (fp16 A), 1 (fp32-faithful) or 2 (fp8 lo planes)");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.prefill(n_tokens, exact == 2 ? 3 : exact ? 2 : 1);
}

int llmi_engine_prefill_scored(llmi_engine* e, int n_tokens, int exact) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_REQUIRE(exact >= 0 && exact <= 2, "prefill: exact must be 0 (fp16 A), 1 (fp32-faithful) or 2 (fp8 lo planes)");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.prefill(n_tokens, exact == 2 ? 3 : exact ? 2 : 1, true);
}

int llmi_engine_scored_logits(llmi_engine* e, int pos, float* out, int n) {
    LLMI_REQUIRE(e, "scored_logits: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.scored_logits_out(pos, out, n);
}

int llmi_engine_sync(llmi_engine* e) {
    LLMI_REQUIRE(e, "null engine");
    LLMI_HIP(hipStreamSynchronize(e->e.stream));
    return LLMI_OK;
}

int llmi_engine_tokens(llmi_engine* e, int32_t* out, int n, int* n_valid) {
    LLMI_REQUIRE(e && (out || n == 0), "null argument");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.tokens_out(out, n, n_valid);
}

int llmi_engine_logits(llmi_engine* e, float* out, int n) {
    LLMI_REQUIRE(e && out && n <= e->e.vl, "engine_logits: bad arguments");
    LLMI_HIP(hipStreamSynchronize(e->e.stream));
    LLMI_HIP(hipMemcpy(out, e->e.logits, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

int llmi_engine_hidden(llmi_engine* e, float* out, int n) {
    LLMI_REQUIRE(e && out && n <= e->e.c.hidden, "engine_hidden: bad arguments");
    LLMI_HIP(hipStreamSynchronize(e->e.stream));
    LLMI_HIP(hipMemcpy(out, e->e.x, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

int llmi_engine_kv_slot(llmi_engine* e, int layer, int pos, int which_v, float* out) {
    LLMI_REQUIRE(e && out, "kv_slot: null argument");
    Engine& g = e->e;
    LLMI_REQUIRE(layer >= 0 && layer < g.c.layers && pos >= 0 && pos < g.c.max_seq, "kv_slot: out of range");
    LLMI_HIP(hipStreamSynchronize(g.stream));
    const size_t eb = llmi::dtype_size(g.c.kv_dtype), D = g.c.head_dim;
    const char* base = g.kv_layer(layer, which_v);
    std::vector<char> tmp(D * eb);
    for (int h = 0; h < g.kvl; ++h) {
        LLMI_HIP(hipMemcpy(tmp.data(), base + ((size_t)h * g.c.max_seq + pos) * D * eb, D * eb,
                           hipMemcpyDeviceToHost));
        float sc = 0.f;
        if (g.c.kv_dtype == LLMI_I8) {  // the cached value: q * s (exact in fp32)
            uint16_t sb = 0;
            LLMI_HIP(hipMemcpy(&sb, g.kv_scale_layer(layer, which_v) + (size_t)h * g.c.max_seq + pos, 2,
                               hipMemcpyDeviceToHost));
            sc = h2f(sb);
        }
        for (size_t d = 0; d < D; ++d) {
            if (g.c.kv_dtype == LLMI_F32)
                std::memcpy(out + h * D + d, tmp.data() + d * 4, 4);
            else if (g.c.kv_dtype == LLMI_I8)
                out[h * D + d] = (float)(int8_t)tmp[d] * sc;
            else
                out[h * D + d] = h2f(*reinterpret_cast<uint16_t*>(tmp.data() + d * 2));
        }
    }
    return LLMI_OK;
}

int llmi_engine_kv_slot_q8(llmi_engine* e, int layer, int pos, int which_v, int8_t* q, uint16_t* scale_bits) {
    LLMI_REQUIRE(e && q && scale_bits, "kv_slot_q8: null argument");
    Engine& g = e->e;
    LLMI_REQUIRE(g.c.kv_dtype == LLMI_I8, "kv_slot_q8: the engine's KV cache is not int8");
    LLMI_REQUIRE(layer >= 0 && layer < g.c.layers && pos >= 0 && pos < g.c.max_seq, "kv_slot_q8: out of range");
    LLMI_HIP(hipStreamSynchronize(g.stream));
    const size_t D = g.c.head_dim;
    LLMI_HIP(hipMemcpy2D(q, D, g.kv_layer(layer, which_v) + (size_t)pos * D, (size_t)g.c.max_seq * D, D, g.kvl,
                         hipMemcpyDeviceToHost));
    LLMI_HIP(hipMemcpy2D(scale_bits, 2, g.kv_scale_layer(layer, which_v) + pos, (size_t)g.c.max_seq * 2, 2, g.kvl,
                         hipMemcpyDeviceToHost));
    return LLMI_OK;
}

int llmi_engine_bytes(llmi_engine* e, uint64_t* weight_bytes, uint64_t* kv_bytes_per_pos) {
    LLMI_REQUIRE(e, "null engine");
    const Engine& g = e->e;
    if (weight_bytes) *weight_bytes = g.stream_bytes;
    if (kv_bytes_per_pos)
        *kv_bytes_per_pos = (uint64_t)g.c.layers * g.kvl * 2 *  // (int8 rows carry an fp16 scale)
                            (g.c.head_dim * llmi::dtype_size(g.c.kv_dtype) + (g.c.kv_dtype == LLMI_I8 ? 2 : 0));
    return LLMI_OK;
}

llmi_stream_t llmi_engine_stream(llmi_engine* e) { return e ? (llmi_stream_t)e->e.stream : nullptr; }

int llmi_engine_xchg_handle(llmi_engine* e, void* out64) {
    LLMI_REQUIRE(e && out64, "xchg_handle: null argument");
    Engine& g = e->e;
    LLMI_REQUIRE(!g.grouped, "xchg_handle: not on a group rank");
    LLMI_HIP(hipSetDevice(g.device));
    LLMI_TRY(g.alloc_xchg());
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle must be 64 bytes");
    hipIpcMemHandle_t h;
    LLMI_HIP(hipIpcGetMemHandle(&h, g.inbox));
    std::memcpy(out64, &h, sizeof(h));
    return LLMI_OK;
}

int llmi_engine_xchg_open(llmi_engine* e, const void* handles) {
    LLMI_REQUIRE(e && handles, "xchg_open: null argument");
    Engine& g = e->e;
    LLMI_REQUIRE(!g.grouped && g.inbox, "xchg_open: call llmi_engine_xchg_handle first");
    LLMI_REQUIRE(!g.peers_ready, "xchg_open: already open");
    LLMI_HIP(hipSetDevice(g.device));
    const int W = g.c.tp_world;
    std::vector<char*> p(W, nullptr);
    for (int q = 0; q < W; ++q) {
        if (q == g.c.tp_rank) {
            p[q] = g.inbox;
            continue;
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, static_cast<const char*>(handles) + (size_t)q * 64, 64);
        void* ptr = nullptr;
        LLMI_HIP(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
        g.peers_opened.push_back(ptr);
        p[q] = static_cast<char*>(ptr);
    }
    LLMI_TRY(g.set_peers(p));
    g.peers_ready = true;
    return LLMI_OK;
}

int llmi_engine_set_option(llmi_engine* e, const char* name, int value) {
    LLMI_REQUIRE(e && name, "set_option: null argument");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_option(name, value);
}

int llmi_engine_xchg_loopback(llmi_engine* e) {
    LLMI_REQUIRE(e, "xchg_loopback: null engine");
    Engine& g = e->e;
    LLMI_REQUIRE(!g.grouped && !g.comm, "xchg_loopback: not on a group rank or an engine with an RCCL communicator");
    LLMI_REQUIRE(!g.peers_ready, "xchg_loopback: the peer exchange is already open");
    LLMI_HIP(hipSetDevice(g.device));
    LLMI_TRY(g.alloc_xchg());
    LLMI_TRY(g.set_peers(std::vector<char*>(g.c.tp_world, g.inbox)));
    g.peers_ready = true;
    g.xchg_loop = 1;
    return LLMI_OK;
}

int llmi_engine_set_decode_mode(llmi_engine* e, int mode) {
    LLMI_REQUIRE(e, "set_decode_mode: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_decode_mode(mode);
}

int llmi_engine_set_exchange(llmi_engine* e, int mode) {
    LLMI_REQUIRE(e, "set_exchange: null engine");
    LLMI_HIP(hipSetDevice(e->e.device));
    return e->e.set_exchange(mode);
}

int llmi_group_set_exchange(llmi_group* g, int mode) {
    LLMI_REQUIRE(g, "group_set_exchange: null group");
    return g->g.set_exchange(mode);
}

int llmi_engine_debug_set_next_pos(llmi_engine* e, int next_pos) {
    LLMI_REQUIRE(e, "debug_set_next_pos: null engine");
    Engine& g = e->e;
    LLMI_HIP(hipSetDevice(g.device));
    LLMI_HIP(hipStreamSynchronize(g.stream));
    LLMI_HIP(hipMemcpy(&g.st->next_pos, &next_pos, sizeof(int), hipMemcpyHostToDevice));
    return LLMI_OK;
}

int llmi_engine_debug_stamps(llmi_engine* e, void* dev_buf) {
    LLMI_REQUIRE(e, "debug_stamps: null engine");
    e->e.dbg_stamps = static_cast<unsigned long long*>(dev_buf);
    return LLMI_OK;
}

int llmi_engine_debug_timeline(llmi_engine* e, void* dev_buf, size_t bytes, int slot_wgs) {
    LLMI_REQUIRE(e, "debug_timeline: null engine");
    Engine& g = e->e;
    LLMI_HIP(hipSetDevice(g.device));
    LLMI_HIP(hipStreamSynchronize(g.stream));  // (also an eager step: the caller may free its last buffer next)
    LLMI_TRY(g.invalidate());  // the captured steps carry the stamp pointers: re-capture
    if (!dev_buf) {
        g.dbg_stamps = nullptr;
        g.dbg_stride = g.dbg_slots = 0;
        return LLMI_OK;
    }
    // every decode launch's grid must fit its region: GEMVs <= 1024 workgroups, attention
    // heads x splits, o_proj heads x (hidden / 16 rows) at most
    const int ns = (g.c.max_seq + llmi::kAttnChunk - 1) / llmi::kAttnChunk;
    const int need = std::max(std::max(1024, g.hl * ns), g.hl * ((g.c.hidden + 15) / 16));
    LLMI_REQUIRE(slot_wgs >= need, "debug_timeline: slot_wgs must be >= " + std::to_string(need));
    g.dbg_stamps = static_cast<unsigned long long*>(dev_buf);
    g.dbg_stride = slot_wgs;
    g.dbg_slots = (int)std::min<size_t>(bytes / ((size_t)slot_wgs * 64), 1 << 20);
    LLMI_REQUIRE(g.dbg_slots > 0, "debug_timeline: buffer smaller than one slot");
    return LLMI_OK;
}

// ---- in-process TP group (single-device parity harness for the sharded path)
int llmi_group_create(const llmi_config* cfg, int world, int device, llmi_group** out) {
    LLMI_REQUIRE(cfg && out, "group_create: null argument");
    *out = nullptr;
    auto h = std::make_unique<llmi_group>();
    int rc = h->g.init(*cfg, world, device);
    if (rc != LLMI_OK) return rc;
    *out = h.release();
    return LLMI_OK;
}

int llmi_group_destroy(llmi_group* g) {
    if (g) {
        (void)hipSetDevice(g->g.r.empty() ? 0 : g->g.r[0]->device);
        (void)hipStreamSynchronize(g->g.stream);
        delete g;
    }
    return LLMI_OK;
}

int llmi_group_load_synthetic(llmi_group* g, uint64_t seed) {
    LLMI_REQUIRE(g, "null group");
    for (auto& e : g->g.r) LLMI_TRY(e->load_synthetic(seed));
    return LLMI_OK;
}

int llmi_group_load_bin(llmi_group* g, const char* weight_path) {
    LLMI_REQUIRE(g, "null group");
    for (auto& e : g->g.r) {
        LLMI_HIP(hipSetDevice(e->device));
        LLMI_TRY(e->load_bin(weight_path));
    }
    return LLMI_OK;
}

int llmi_group_load_bin_quantized(llmi_group* g, const char* weight_path) {
    LLMI_REQUIRE(g, "null group");
    for (auto& e : g->g.r) {
        LLMI_HIP(hipSetDevice(e->device));
        LLMI_TRY(e->load_bin(weight_path, true));
    }
    return LLMI_OK;
}

int llmi_group_set_prompt(llmi_group* g, const int32_t* ids, int n) {
    LLMI_REQUIRE(g, "null group");
    for (auto& e : g->g.r) LLMI_TRY(e->set_prompt(ids, n));
    return LLMI_OK;
}

int llmi_group_decode(llmi_group* g, int n_steps, int use_graph) {
    LLMI_REQUIRE(g, "null group");
    return g->g.decode(n_steps, use_graph);
}

int llmi_group_tokens(llmi_group* g, int rank, int32_t* out, int n, int* n_valid) {
    LLMI_REQUIRE(g && (out || n == 0) && rank >= 0 && rank < (int)g->g.r.size(), "group_tokens: bad arguments");
    return g->g.r[rank]->tokens_out(out, n, n_valid);
}

int llmi_group_logits(llmi_group* g, float* out, int n) {
    LLMI_REQUIRE(g && out, "group_logits: null argument");
    LLMI_HIP(hipStreamSynchronize(g->g.stream));
    int off = 0;
    for (auto& e : g->g.r) {  // vocab-parallel slices in rank order = the full vocab
        const int m = std::min(e->vl, n - off);
        if (m <= 0) break;
        LLMI_HIP(hipMemcpy(out + off, e->logits, (size_t)m * 4, hipMemcpyDeviceToHost));
        off += m;
    }
    return LLMI_OK;
}

int llmi_group_hidden(llmi_group* g, int rank, float* out, int n) {
    LLMI_REQUIRE(g && out && rank >= 0 && rank < (int)g->g.r.size() && n <= g->g.r[0]->c.hidden,
                 "group_hidden: bad arguments");
    LLMI_HIP(hipStreamSynchronize(g->g.stream));
    LLMI_HIP(hipMemcpy(out, g->g.r[rank]->x, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

// ---- batched decode (struct Batch)
int llmi_batch_create(const llmi_config* cfg, int n_seq, int device, llmi_batch** out) {
    LLMI_REQUIRE(cfg && out, "batch_create: null argument");
    *out = nullptr;
    auto h = std::make_unique<llmi_batch>();
    int rc = h->b.init(*cfg, n_seq, device);
    if (rc != LLMI_OK) return rc;
    *out = h.release();
    return LLMI_OK;
}

int llmi_batch_destroy(llmi_batch* b) {
    if (b) {
        (void)hipSetDevice(b->b.r.empty() ? 0 : b->b.r[0]->device);
        if (b->b.stream) (void)hipStreamSynchronize(b->b.stream);
        delete b;
    }
    return LLMI_OK;
}

int llmi_batch_load_synthetic(llmi_batch* b, uint64_t seed) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    LLMI_TRY(b->b.r[0]->load_synthetic(seed));
    return b->b.loaded();
}

int llmi_batch_load_bin(llmi_batch* b, const char* weight_path) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    LLMI_TRY(b->b.r[0]->load_bin(weight_path));
    return b->b.loaded();
}

int llmi_batch_load_bin_quantized(llmi_batch* b, const char* weight_path) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    LLMI_TRY(b->b.r[0]->load_bin(weight_path, true));
    return b->b.loaded();
}

int llmi_batch_set_prompt(llmi_batch* b, int seq, const int32_t* ids, int n) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->set_prompt(ids, n);
}

int llmi_batch_edit(llmi_batch* b, int seq, int keep, const int32_t* ids, int n) {
    LLMI_REQUIRE(b, "batch_edit: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->edit(keep, ids, n);  // (an idle slot has no prompt: LLMI_EINVAL)
}

int llmi_batch_fork(llmi_batch* b, int src, const int* dst, int n_dst, int keep, const int32_t* ids, int n) {
    LLMI_REQUIRE(b, "batch_fork: null batch");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.fork(src, dst, n_dst, keep, ids, n);
}

int llmi_batch_reset(llmi_batch* b, int seq) {
    LLMI_REQUIRE(b, "null batch");
    return b->b.reset(seq);
}

int llmi_batch_set_sampling_params(llmi_batch* b, int seq, const llmi_sampling_params* p) {
    LLMI_REQUIRE(b && p, "batch_set_sampling_params: null batch or params");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->set_sampling_params(*p);
}

// The slot's own engine setters: wherever one drops the engine's captured steps it drops the
// batch's (Engine::invalidate).
int llmi_batch_set_logit_rules(llmi_batch* b, int seq, const int32_t* bias_ids, const float* bias_values, int n_bias,
                               float presence_penalty, float frequency_penalty, int count_prompt) {
    LLMI_REQUIRE(b, "batch_set_logit_rules: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->set_logit_rules(bias_ids, bias_values, n_bias, presence_penalty, frequency_penalty,
                                        count_prompt);
}

int llmi_batch_set_allowed(llmi_batch* b, int seq, const int32_t* ids, int n) {
    LLMI_REQUIRE(b, "batch_set_allowed: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->set_allowed(ids, n);
}

int llmi_batch_clear_logit_rules(llmi_batch* b, int seq) {
    LLMI_REQUIRE(b, "batch_clear_logit_rules: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->clear_logit_rules();
}

int llmi_batch_processed_logits(llmi_batch* b, int seq, float* out, int n) {
    LLMI_REQUIRE(b, "batch_processed_logits: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->processed_out(out, n);
}

int llmi_batch_set_logprobs(llmi_batch* b, int seq, int n_top) {
    LLMI_REQUIRE(b, "batch_set_logprobs: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->set_logprobs(n_top);
}

int llmi_batch_logprobs(llmi_batch* b, int seq, float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid,
                        int* n_top) {
    LLMI_REQUIRE(b, "batch_logprobs: null batch");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.r[seq]->logprobs_out(tok_lp, top_ids, top_lp, n, n_valid, n_top);
}

int llmi_batch_decode(llmi_batch* b, int n_steps, int use_graph) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.decode(n_steps, use_graph);
}

int llmi_batch_prefill(llmi_batch* b, int seq, int n_tokens, int exact, int scored) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_REQUIRE(exact >= 0 && exact <= 2, "prefill: exact must be 0 (fp16 A), 1 (fp32-faithful) or 2 (fp8 lo planes)");
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    return b->b.prefill(seq, n_tokens, exact == 2 ? 3 : exact ? 2 : 1, scored != 0);
}

int llmi_batch_tokens(llmi_batch* b, int seq, int32_t* out, int n, int* n_valid) {
    LLMI_REQUIRE(b && (out || n == 0), "batch_tokens: null argument");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_HIP(hipSetDevice(b->b.r[0]->device));
    if (b->b.r[seq]->prompt_len == 0) {  // idle: no sequence
        if (n_valid) *n_valid = 0;
        return LLMI_OK;
    }
    return b->b.r[seq]->tokens_out(out, n, n_valid);
}

int llmi_batch_logits(llmi_batch* b, int seq, float* out, int n) {
    LLMI_REQUIRE(b && out, "batch_logits: null argument");
    LLMI_TRY(b->b.slot_ok(seq));
    LLMI_REQUIRE(n >= 0 && n <= b->b.r[seq]->vl, "batch_logits: n exceeds the vocabulary");
    LLMI_HIP(hipStreamSynchronize(b->b.stream));
    LLMI_HIP(hipMemcpy(out, b->b.r[seq]->logits, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

int llmi_batch_sync(llmi_batch* b) {
    LLMI_REQUIRE(b, "null batch");
    LLMI_HIP(hipStreamSynchronize(b->b.stream));
    return LLMI_OK;
}

int llmi_batch_bytes(llmi_batch* b, uint64_t* weight_bytes_per_step, uint64_t* kv_bytes_per_pos) {
    LLMI_REQUIRE(b, "null batch");
    const Engine& g = *b->b.r[0];
    const uint64_t n_act = b->b.active().size();
    // the weights once; W_o (+ its int8 row scales) once more for every further active slot
    const uint64_t wo = Engine::lin_bytes(g.odt(), g.c.hidden, g.ql) + Engine::scale_bytes(g.odt(), g.c.hidden, g.ql);
    if (weight_bytes_per_step)
        *weight_bytes_per_step = g.stream_bytes + (n_act > 1 ? (n_act - 1) * wo * g.c.layers : 0);
    if (kv_bytes_per_pos)
        *kv_bytes_per_pos = (uint64_t)g.c.layers * g.kvl * 2 *  // (int8 rows carry an fp16 scale)
                            (g.c.head_dim * llmi::dtype_size(g.c.kv_dtype) + (g.c.kv_dtype == LLMI_I8 ? 2 : 0));
    return LLMI_OK;
}

}  // extern "C"
