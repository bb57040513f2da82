// DecodeEngine: the Llama<T> single-stream greedy decode loop on one GPU (or
// one tensor-parallel rank), as one hipGraph per token.
//
// Reference call stack replaced:
//   Llama<T>::Response / continueTokenGen       src/models/llama/llama.cpp:318-349, 362-457
//   LlamaSelfDecoder<T>::forward                src/layers/decoder/self_decoder.cpp:23-89
//   LLaMASelfAttentionLayer<T>::Forward         src/layers/attention/masked_self_attention.cpp:54-92
//   LLaMAFFNLayer<T>::forward                   src/layers/ffn/ffn.cpp:52-93
//   LMHeadAndTopKSample                         src/models/llama/llama.cpp:214-269
// The reference issues ~326 launches per token, each followed by
// cudaDeviceSynchronize, plus a D2H and an H2D copy per token. Here one token is
//   step_start (token pick + embedding)
//   L x [ rmsnorm+QKV gemv | rope+kv-write+split-KV attention | O gemv+residual
//         (| allreduce) | rmsnorm+gate_up gemv+silu*mul | down gemv+residual (| allreduce) ]
//   final rmsnorm + lm_head gemv + argmax partials (| allreduce max)
// = 5L + 2 kernels, captured once into a hipGraph; positions, token ids and the
// argmax hand-off live in device memory, so tokens are produced with no host sync.
//
// HBM layout (one allocation each): all weights contiguous per layer in
// forward order (qkv, o, gate_up, down, norms), then lm_head, final norm,
// embedding; KV cache [layers, kv_heads, max_seq, head_dim] per K and V
// (concat_past_kv.cu:122 layout, batch 1); fp32 activations (16-44 KB) and
// the decode state in a small scratch block.
//
// Tensor parallel: Megatron column/row split over tp_world
// ranks, one process per GPU; q/k/v and gate/up rows split by heads / inter
// columns, o and down split on their input columns. Rank 0 adds the residual
// in the o/down epilogue, every other rank stores its bare partial, and an RCCL
// all-reduce(sum) over xGMI yields residual + sum of partials in place: 2 per
// layer. The vocab-parallel lm_head produces per-workgroup argmax keys with
// global row ids; an all-reduce(max) of the keys gives every rank the same
// next token. Weights are generated shard-by-shard from the same global PRNG
// indices, so every TP degree computes the same model.
//
// Captured steps: who owns them, what invalidates them. Every captured step lives in a
// GraphCache of the object that launches it: an Engine's token steps (by split count) and its
// verify steps (by rows and split count), a Group's steps, a Batch's steps (by the active slots
// and their split counts). A key carries only what changes without a setter call; whatever a
// setter changes in a recorded step goes through Engine::invalidate(), which drops the engine's
// own caches and those of the owner whose steps hold this engine's launches (a slot's batch, a
// verify lane's engine). A Group drops its own cache in Group::set_exchange. Replacing the
// contents of an allowed-token mask that is already present is a stream-ordered copy into a
// fixed buffer and invalidates nothing. Neither does a fork (Engine::fork_into, Batch::fork): a
// batch step's key is (slot, split count) and its launches hold the slot's own buffers, none of
// which move; the fork only writes their contents, in stream order (as set_prompt and edit do).
//
// One struct Engine, defined over several units: engine_weights.hip (setup and the
// loaders), engine.hip (the token step, the TP exchange, the ring layer, the setters),
// engine_prefill.hip, engine_spec.hip (the verify step, the lookup and draft-engine loops),
// engine_edit.hip (rewind / extend a sequence), engine_fork.hip (copy a sequence into other
// slots; the cache rows through kv_fork.hip), engine_group.hip / engine_batch.hip (Group,
// Batch), engine_capi.hip (the C ABI) and engine_time.hip (llmi_engine_time_kernel).
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include <string>

#include "kernels.h"

// compile-time defaults, here only: every unit sees the same value under LLMI_EXTRA_CFLAGS
#ifndef LLMI_F16_DOWN_KSPLIT
#define LLMI_F16_DOWN_KSPLIT 1  // fp16 down K slices (int64 atomics: exact in any order)
#endif
#ifndef LLMI_I8_DOWN_KSPLIT
#define LLMI_I8_DOWN_KSPLIT 4  // int8 down K slices: 13B down 18.2 -> 16.5 us, 8-layer loop 682 -> 665 us (A/B)
#endif
#ifndef LLMI_QKV_ATTN
#define LLMI_QKV_ATTN 1  // one q/k/v GEMV + attention launch (qkv_attn.hip); engine option "qkv_attn"
#endif
#ifndef LLMI_QKV_ATTN_O
#define LLMI_QKV_ATTN_O 0  // the fused launch also runs the o_proj (fp16 MHA, single rank); option "qa_o"
#endif

namespace llmi {

// Offsets into one allocation: take() hands out consecutive blocks, each starting on a
// 256-byte boundary; off is the size to allocate.
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) / 256 * 256;
        return o;
    }
};

// Capture record() on s into a graph and instantiate it. The capture is always ended, also
// when record() failed (a stream left capturing is unusable); the graph is destroyed when
// record() or the instantiate failed, and *graph / *exec are written only on full success.
template <typename F>
int capture(hipStream_t s, F&& record, hipGraph_t* graph, hipGraphExec_t* exec) {
    LLMI_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = record();
    hipGraph_t h = nullptr;
    hipError_t e = hipStreamEndCapture(s, &h);
    hipGraphExec_t x = nullptr;
    if (rc == LLMI_OK && e == hipSuccess) e = hipGraphInstantiate(&x, h, nullptr, nullptr, 0);
    if (rc != LLMI_OK || e != hipSuccess) {
        if (h) (void)hipGraphDestroy(h);
        LLMI_TRY(rc);
        LLMI_HIP(e);
    }
    *graph = h;
    *exec = x;
    return LLMI_OK;
}

// The captured steps of one owner (an Engine's token steps and its verify steps, a Group's, a
// Batch's), by key, built lazily. The attention and o_proj grids are sized on the host
// (AttnArgs::nact = pos / 64 + 1), so a captured step is valid for 64 consecutive positions and
// every key carries the split count(s). The cache owns the graphs and their execs. bound > 0: a
// full cache is dropped whole (after a stream sync) before the next capture.
template <typename Key>
struct GraphCache {
    std::map<Key, std::pair<hipGraph_t, hipGraphExec_t>> m;
    size_t bound;
    explicit GraphCache(size_t bound_ = 0) : bound(bound_) {}
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() { clear(); }
    void clear() {  // (the caller knows that no replay is in flight)
        for (auto& kv : m) {
            (void)hipGraphExecDestroy(kv.second.second);
            (void)hipGraphDestroy(kv.second.first);
        }
        m.clear();
    }
    // what every invalidation is: a replay may still be in flight, so synchronise, then clear
    int drop(hipStream_t s) {
        if (m.empty()) return LLMI_OK;
        LLMI_HIP(hipStreamSynchronize(s));
        clear();
        return LLMI_OK;
    }
    // *exec = the step of `key`, captured with record() on s where the cache has none; a failed
    // capture leaves no entry (and, capture(): no stream stuck in capture mode)
    template <typename F>
    int get(const Key& key, hipStream_t s, F&& record, hipGraphExec_t* exec) {
        auto it = m.find(key);
        if (it == m.end()) {
            if (bound && m.size() >= bound) LLMI_TRY(drop(s));
            hipGraph_t h = nullptr;
            hipGraphExec_t x = nullptr;
            LLMI_TRY(capture(s, record, &h, &x));
            it = m.emplace(key, std::make_pair(h, x)).first;
        }
        *exec = it->second.second;
        return LLMI_OK;
    }
};
using BatchGraphs = GraphCache<std::vector<int>>;

// One multi-row GEMV from the single-row arguments args_of(engine) of up to kGemvRowsMax engines
// (a batch's active slots, a verify step's lanes): the launch takes the first engine's weights
// and shape and every engine's own row pointers. with_stamps false: it writes no debug stamps.
struct Engine;
template <typename F>
int gemv_rows_of(const std::vector<Engine*>& es, hipStream_t s, F&& args_of, bool with_stamps = true) {
    GemvRowsArgs p;
    for (Engine* e : es) gemv_rows_add(p, args_of(*e));
    if (!with_stamps) p.a.stamps = nullptr;
    return gemv_rows_launch(p, s);
}

// The modes of an engine that refuse one another (Engine::refuse; engine.hip has the table). The
// first four are fixed when the engine is made; the rest are turned on and off by setters.
enum Mode { kModeTp, kModeSlot, kModeInt4, kModeKv8, kModeRing, kModeTopK, kModeNucleus, kModeLogprobs, kModeRules,
            kModeSpec };

// "<n> (1: ..., 2: ...)": a DecodeState::error word and the legend of its bits
std::string error_flag_text(int flags);

struct Engine {
    llmi_config c{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;  // false inside an in-process group (the group's stream)
    bool grouped = false;    // rank of an in-process TP group: reductions are the group's
    // local (per-rank) dims
    int hl = 0, kvl = 0, ql = 0, kvrows = 0, il = 0, vl = 0;
    int wdt = LLMI_F16;      // linear weight dtype
    int edt = LLMI_F16;      // embedding / lm_head / norm dtype
    size_t wsz = 2, esz = 2;  // (wsz 0 for int4: weight sizes go through lin_bytes)
    // int4 engines keep W_o W8A16 (8.3 % of a layer; the o_proj kernel's 16-lane head slices)
    int odt() const { return wdt == LLMI_I4 ? LLMI_I8 : wdt; }
    bool quantised() const { return wdt == LLMI_I8 || wdt == LLMI_I4; }
    // bytes of a [rows, cols] linear weight of dtype dt, and of its fp16 scales (int8: one a
    // row; int4: one a 128-column group)
    static uint64_t lin_bytes(int dt, uint64_t rows, uint64_t cols) { return rows * row_bytes(dt, cols); }
    static uint64_t scale_bytes(int dt, uint64_t rows, uint64_t cols) {
        return dt == LLMI_I8 ? rows * 2 : dt == LLMI_I4 ? rows * (cols / 128) * 2 : 0;
    }
    int n_cu = 0;
    uint64_t seed = 0;

    // ------------------------------------------------------------ weights
    struct Layer {
        void *qkv = nullptr, *o = nullptr, *gu = nullptr, *down = nullptr;
        __half *qkv_s = nullptr, *o_s = nullptr, *gu_s = nullptr, *down_s = nullptr;
        void *attn_norm = nullptr, *ffn_norm = nullptr;
    };
    std::vector<Layer> layers;
    void *embed = nullptr, *lm_head = nullptr, *final_norm = nullptr;
    char* wblob = nullptr;
    size_t wbytes = 0;
    uint64_t stream_bytes = 0;  // weight bytes one forward reads

    // ----------------------------------------------------------------- KV
    void *kcache = nullptr, *vcache = nullptr;
    size_t kv_layer_elems = 0;
    // int8 cache (KV8, include/llmi.h): one fp16 scale per cached row [layers, kv_heads, max_seq],
    // carved from the same allocation after the bytes (256-byte aligned); null otherwise
    __half *kscale = nullptr, *vscale = nullptr;
    static size_t kv_align(size_t n) { return (n + 255) & ~(size_t)255; }
    size_t kv_data_bytes() const { return (size_t)c.layers * kv_layer_elems * dtype_size(c.kv_dtype); }
    size_t kv_scale_bytes() const { return c.kv_dtype == LLMI_I8 ? (size_t)c.layers * kvl * c.max_seq * 2 : 0; }
    // one allocation (K or V): the rows, then the scales
    size_t kv_alloc_bytes() const { return kv_scale_bytes() ? kv_align(kv_data_bytes()) + kv_scale_bytes() : kv_data_bytes(); }
    __half* kv_scale_layer(int l, int which_v) const {
        __half* b = which_v ? vscale : kscale;
        return b ? b + (size_t)l * kvl * c.max_seq : nullptr;
    }
    // layer l's K (or V) cache [kv_heads, max_seq, head_dim]
    char* kv_layer(int l, int which_v) const {
        return (char*)(which_v ? vcache : kcache) + (size_t)l * kv_layer_elems * dtype_size(c.kv_dtype);
    }

    // ------------------------------------------------------------ scratch
    char* scratch = nullptr;
    float *x = nullptr, *qkv_buf = nullptr, *attn_out = nullptr, *act = nullptr, *logits = nullptr;
    // Residual stream in int64 fixed point (value * 2^32): res[l % 2] is layer l's input,
    // xacc the mid-layer accumulator (residual + o_proj), res[(l + 1) % 2] the output
    // (mid + down). Every residual add is an exact integer add, so sums are
    // independent of workgroup order and of the TP reduction order.
    long long* xacc = nullptr;
    long long* res[2] = {nullptr, nullptr};
    unsigned long long* partials = nullptr;
    int lm_grid = 0;
    void* attn_ws = nullptr;
    float* rope_tab = nullptr;  // [max_seq][head_dim/2] (cos, sin): modeling_llama.py:130-146 cache
    DecodeState* st = nullptr;
    int32_t *prompt = nullptr, *tokens = nullptr;
    int host_next_pos = 0, prompt_len = 0;

    GraphCache<int> graphs;  // the token steps, by split count
    // a batch slot: the batch's captured steps, which hold this engine's launches (Batch::init)
    BatchGraphs* owner_graphs = nullptr;
    int rec_nact = 0;  // active split count the next recorded step's attention is sized for
    // fused q/k/v + attention launch (qkv_attn.hip) where the shapes allow it; option "qkv_attn",
    // default LLMI_QKV_ATTN (A/B); qtag: its granule buffer [(heads + 2 kv) * d]
    bool qa_fuse = LLMI_QKV_ATTN != 0;
    bool qa_o = LLMI_QKV_ATTN_O != 0;  // ... with the o_proj in the same launch (option "qa_o")
    unsigned long long* qtag = nullptr;
    bool kpar_off = false;  // option "kpar" 0

    // -------------------------------------------------------- TP exchange
    ncclComm_t comm = nullptr;
    // one-shot peer exchange (xchg.hip): this rank's inbox (uncached HBM), every rank's
    // inbox base (IPC-mapped for peers) in device memory, per-slice epoch counters.
    // xchg_mode 1 replaces the RCCL all-reduces of the token graph (RCCL stays selectable);
    // xchg_mode 2 moves the exchange into the producing launches (o_proj, down, lm_head
    // finish with xchg_tail: push + wait + reduce, no exchange launch). tail_mode: what
    // those launches do (0 nothing, 1 push only -- the in-process group, 3 push + reduce);
    // xt_cnt their arrival counters (xchg_impl.h: sharded, zeroed here, re-zeroed by every
    // fused launch's finishers).
    int xchg_mode = 0;
    int tail_mode = 0;
    unsigned* xt_cnt = nullptr;
    char* inbox = nullptr;
    char** peers_dev = nullptr;
    unsigned long long* xchg_ep = nullptr;
    std::vector<void*> peers_opened;  // IPC mappings to close
    int xchg_cap_n = 0;
    bool peers_ready = false;
    int xchg_loop = 0;  // llmi_engine_xchg_loopback: one rank alone, every peer its own inbox

    // ------------------------------------------------------------ prefill
    static constexpr int kPrefillRows = 512;
    // prefill scratch (allocated on first use): rows of one prefill chunk
    char* pf = nullptr;
    int pf_rows = 0;
    float *pf_x = nullptr, *pf_qkv = nullptr, *pf_o = nullptr, *pf_act = nullptr;
    _Float16 *pf_ah = nullptr, *pf_al = nullptr;  // fp16 activation planes (gemm2 path)
    float* pf_slab = nullptr;      // split-K partial slabs of the o_proj / down GEMMs [kPfSlabs][R][H]
    float* pf_split = nullptr;     // split-key prefill attention partials
    size_t pf_split_floats = 0;
    int pf_pending = 0;            // slices in pf_slab not yet added into pf_x
    static constexpr int kPfSplit = 2;   // o_proj (gemm2) K slices
    static constexpr int kPfDown = 8;    // down (gemm3) K slices
    static constexpr int kPfSlabs = 8;
    // split mode 3: e4m3 copies of the prefill GEMM weights (W * 2^exp, gemm3.hip), made on first use
    struct W8Layer {
        void *qkv = nullptr, *o = nullptr, *gu = nullptr, *down = nullptr;
        int qkv_e = 0, o_e = 0, gu_e = 0, down_e = 0;
    };
    std::vector<W8Layer> w8l;
    char* w8blob = nullptr;
    // the SiLU output planes reuse pf_act's bytes (fp32 [R, il] = two fp16 planes)
    _Float16* pf_act_h() { return reinterpret_cast<_Float16*>(pf_act); }
    _Float16* pf_act_l() { return reinterpret_cast<_Float16*>(pf_act) + (size_t)pf_rows * il; }
    // scored prefill: fp32 logits of one chunk's rows [pf_rows][vocab] (allocated on first use,
    // never touched by the plain prefill), and the prompt rows [sc_p0, sc_p0 + sc_m) the last
    // scored chunk's lm_head GEMM left there
    float* sc_logits = nullptr;
    int sc_p0 = 0, sc_m = 0;
    // a batch slot borrows slot 0's prefill scratch, e4m3 weight copies and logits slab (the
    // pointers above are copies taken at every prefill; nothing of them is freed by the slot)
    Engine* pf_from = nullptr;

    // --------------------------------------------------------------- ring
    // decode mode 1: the persistent ring layer (ring.hip) -- per token step_start, q/k/v(0),
    // L x [attention, ring], lm_head. rl_acc holds the int64 residual accumulators in
    // five slots [A0][A1][B0][A2][B1] (A: layer inputs x_l, slot l % 3; B: mid-layer sums,
    // slot l % 2), A1 + B0 adjacent so step_start zeroes both; rl_cnt the per-layer fan-in
    // counters; wdt the transposed W_down copies the ring's K split reads.
    int decode_mode = 0;
    long long* rl_acc = nullptr;
    unsigned* rl_cnt = nullptr;
    char* wdt_blob = nullptr;
    bool wdt_valid = false;
    long long* acc_a(int l) const { static const int s[3] = {0, 1, 3}; return rl_acc + (size_t)s[l % 3] * c.hidden; }
    long long* acc_b(int l) const { return rl_acc + (size_t)(l % 2 ? 4 : 2) * c.hidden; }
    void* wdt_of(int l) const { return wdt_blob + (size_t)l * il * c.hidden * 2; }

    // --------------------------------------------- quantised-load staging
    // quantised loads (load_tensor with quantize): fp32 staging rows for quant.hip, the bad-row
    // counter in its first 256 bytes; lives for one load (qstage_hold: a load_bin spans tensors)
    char* qstage = nullptr;
    size_t qstage_bytes = 0;
    bool qstage_hold = false;
    static constexpr size_t kQStageBytes = (size_t)256 << 20;
    static constexpr size_t kQStageHead = 256;  // the bad-row counter, then 16-byte aligned rows

    // ----------------------------------------------------------- sampling
    // stochastic sampling (Llama<T>::Sampling, llama.cpp:245-262): 0 = greedy argmax
    int sample_k = 0;
    uint64_t sample_seed = 0;
    // llmi_engine_set_sampling_params: the nucleus sampler (nucleus.hip) instead
    bool nuc_on = false;
    llmi_sampling_params nuc{};
    int32_t* samp_ids = nullptr;
    float* samp_vals = nullptr;

    // ----------------------------------------------------------- logprobs
    // llmi_engine_set_logprobs: -1 off, else the alternatives per record; one blob of
    // max_seq + 1 records each of tok_lp, top_ids [kLpMaxTop], top_lp [kLpMaxTop] (the two
    // top arrays are indexed with stride lp_top), 0xFF-filled = "not computed"
    static constexpr int kLpMaxTop = 8;
    int lp_top = -1;
    int lp_stride = -1;  // the n_top the records were laid out for (kept while off)
    char* lp_buf = nullptr;
    size_t lp_records() const { return (size_t)c.max_seq + 1; }
    size_t lp_bytes() const { return lp_records() * 4 * (1 + 2 * kLpMaxTop); }
    float* lp_tok() const { return reinterpret_cast<float*>(lp_buf); }
    int32_t* lp_ids() const { return reinterpret_cast<int32_t*>(lp_buf + lp_records() * 4); }
    float* lp_tlp() const { return reinterpret_cast<float*>(lp_buf + lp_records() * 4 * (1 + kLpMaxTop)); }

    // -------------------------------------------------------- logit rules
    // llmi_engine_set_logit_rules / llmi_engine_set_allowed: one launch (logit_rules.hip, engine
    // form) after the lm_head and before the sampler, which then reads lr_out instead of logits.
    // lr_allowed is carved from scratch at setup and holds all ones while no mask is set, so a
    // mask's contents change with a stream-ordered copy and never with the launch arguments;
    // lr_bias (dense [vocab]) and lr_out (the processed row [vocab]) are this engine's own
    // allocations, made by the first setter that needs them and freed in ~Engine.
    uint32_t* lr_allowed = nullptr;
    float *lr_bias = nullptr, *lr_out = nullptr;
    bool lr_bias_on = false, lr_mask_on = false;
    float lr_presence = 0.f, lr_frequency = 0.f;
    int lr_count_prompt = 0;
    size_t lr_words() const { return ((size_t)c.vocab + 31) / 32; }
    bool rules_on() const { return lr_bias_on || lr_mask_on || lr_presence != 0.f || lr_frequency != 0.f; }

    // -------------------------------------------------------- speculation
    // llmi_engine_set_speculation (engine_spec.hip): spec_max extra lanes, each an Engine on this
    // stream that borrows the weights (init's lender) and -- kv_from -- the KV cache and the RoPE
    // table, with its own DecodeState, x, q/k/v, activations, residual accumulators, attention
    // workspace, logits and argmax partials. spec_draft: device [8] draft ids, then {a, g_a, error}.
    // spec_graphs: captured verify steps by (rows, split count of the last row). A lane's
    // kv_from is its engine, whose verify steps hold the lane's launches.
    Engine* kv_from = nullptr;
    int spec_max = 0;
    std::vector<std::unique_ptr<Engine>> lanes;
    int32_t* spec_draft = nullptr;
    static constexpr size_t kMaxSpecGraphs = 64;
    GraphCache<std::pair<int, int>> spec_graphs{kMaxSpecGraphs};

    // -------------------------------------------------------------- debug
    unsigned long long* dbg_stamps = nullptr;  // llmi_engine_debug_stamps: per-workgroup timeline
    // llmi_engine_debug_timeline: every stamped launch of a recorded step gets its own
    // region of dbg_stride workgroups (slot = launch order), dbg_slots regions in all
    int dbg_stride = 0, dbg_slots = 0;
    mutable int dbg_slot = 0;
    unsigned long long* stamp_ptr() const {
        if (!dbg_stamps || dbg_stride == 0) return dbg_stamps;
        const int s = dbg_slot++;
        return s < dbg_slots ? dbg_stamps + (size_t)s * dbg_stride * 8 : nullptr;
    }

    // ---- engine_weights.hip: setup, teardown and the loaders
    ~Engine();
    int init(const llmi_config& cfg, int dev, const void* tp_id, hipStream_t ext_stream = nullptr,
             const Engine* lender = nullptr, bool group_rank = true);
    int alloc_weights();
    int alloc_state();
    int weights_changed();
    int load_synthetic(uint64_t sd);
    int load_synthetic_i4();
    static int put_host(void* dst, int dt, const float* src, size_t src_ld, int rows, int cols, size_t row0,
                        size_t col0, hipStream_t s);
    void quant_release();
    int quant_stage(size_t row_bytes, int rows, int* chunk);
    int quant_rows(const float* rows_dev, size_t ld, int n, int cols, void* q_dst, __half* s_dst, size_t q_row, int qdt,
                   int32_t* bad, int col0 = 0);
    int quant_put(const std::string& nm, const float* src, size_t src_ld, size_t row0, int rows, int col0, int cols,
                  void* q_dst, size_t q_row_off, __half* s_dst, int qdt);
    int load_tensor(const char* name, const float* src, size_t count, bool quantize = false);
    int load_tensor_impl(const char* name, const float* src, size_t count, bool quantize);
    int load_bin(const char* weight_path, bool quantize = false);
    int load_bin_impl(const char* weight_path, bool quantize);

    // ---- engine.hip: the token step
    GemvArgs lm_args(bool from_x = false) const;
    int kpar_of(int groups) const;
    GemvArgs qkv_args(int l) const;
    AttnArgs attn_args(int l) const;
    OprojArgs o_args(int l) const;
    GemvArgs gu_args(int l) const;
    GemvArgs down_args(int l) const;
    int down_ksplit() const;
    bool down_single() const;
    bool seed_from_down() const;
    void tag_qkv(GemvArgs& q, AttnArgs& at, int l) const;
    int rec_start();
    int rec_attn(int l);
    int rec_oproj(int prev, OprojArgs o, const AttnArgs* at = nullptr);
    int rec_ffn(int l);
    int rec_head(bool from_x = false);
    int rec_sample();
    int rec_pick();
    int rec_logprob();
    int record_step();
    static int nact_of(int pos) { return pos / kAttnChunk + 1; }
    int build_graph(int nact, hipGraphExec_t* exec);
    int invalidate();
    int set_prompt(const int32_t* ids, int n);
    int decode(int n, int use_graph);
    int tokens_out(int32_t* out, int n, int* n_valid);
    // ... the TP exchange
    int alloc_xchg();
    int set_peers(const std::vector<char*>& p);
    XchgArgs xchg_args(void* buf, int n, int op, int mode) const;
    int exchange(void* buf, int n, int op);
    int set_exchange(int mode);
    // ... which mode refuses which
    static unsigned config_modes(const llmi_config& cfg);
    unsigned modes() const;
    static int refuse(const char* who, Mode turning_on, unsigned on);
    int refuse(const char* who, Mode turning_on) const { return refuse(who, turning_on, modes()); }
    // ... the option, sampling and logprob setters
    int set_option(const std::string& name, int value);
    int set_sampling(int k, uint64_t sd);
    int set_sampling_params(const llmi_sampling_params& p);
    int set_logprobs(int n_top);
    int logprobs_out(float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid, int* n_top);
    // ... the logit rules
    int rules_turn_on();
    int set_logit_rules(const int32_t* bias_ids, const float* bias_values, int n_bias, float presence, float frequency,
                        int count_prompt);
    int set_allowed(const int32_t* ids, int n);
    int clear_logit_rules();
    int processed_out(float* out, int n);
    // ... the ring layer
    bool ring_ok() const;
    int set_decode_mode(int mode);
    int prepare_ring();
    RingArgs ring_args(int l, bool wrap = false) const;
    int record_step_ring();

    // ---- engine_prefill.hip
    int alloc_prefill();
    bool lo8_supported() const;
    int alloc_w8();
    PrefillAttnArgs prefill_attn_args(int l, int m, int p0) const;
    int prefill_layer_gemm2(int l, int m, int p0, int split);
    int prefill_flush(int m);
    int alloc_score();
    int prefill_scratch(int split, bool scored);
    bool head_gemm_supported(bool use_gemm2) const;
    int score_chunk(int m, int p0, int split, bool use_gemm2, bool last);
    int prefill(int n, int split, bool scored = false);
    int scored_logits_out(int pos, float* out, int n);

    // ---- engine_spec.hip: speculative decoding (the verify step, the lookup generation loop)
    int set_speculation(int max_draft);
    int record_verify(int m);
    int verify(const int32_t* draft, int n_draft, int use_graph, int* n_accepted, int* next_token = nullptr);
    int generate_lookup(int n_steps, int max_draft, int ngram_max, int ngram_min, int use_graph,
                        llmi_spec_stats* stats);
    // ... a second engine proposes (this one is the target)
    int read_ids(int from, int n, int32_t* out);
    int draft_catch_up(const int32_t* hist, int p, int use_prefill, int use_graph);
    int generate_draft(Engine& draft, int n_steps, int max_draft, int draft_prefill, int use_graph,
                       llmi_spec_stats* stats);

    // ---- engine_edit.hip: keep a prefix of the sequence, force the ids that follow
    int edit(int keep, const int32_t* ids, int n);

    // ---- engine_fork.hip: copy this sequence into other engines on this stream (a batch's slots),
    // cut at `keep` with forced ids as edit would (n >= 1), or as it stands (n == 0, keep == position)
    int fork_into(const std::vector<Engine*>& dst, int keep, const int32_t* ids, int n);
};
// prompt-lookup drafting on the host (llmi_lookup_draft)
int lookup_draft(const int32_t* ids, int n, int ngram_max, int ngram_min, int max_draft, int32_t* out, int* n_out);

// In-process tensor-parallel group: W rank engines (tp_rank 0..W-1) on ONE
// device and ONE stream, stepped phase by phase with group_reduce_kernel in
// place of the RCCL all-reduces. RCCL refuses two ranks on one device, so this
// is how the sharded path (per-rank weights, rank-0 residual, vocab-parallel
// argmax keys) is parity-tested on a single GPU; numerically it differs from
// the RCCL path only in the fp32 summation order of the down-proj partials.
struct Group {
    std::vector<std::unique_ptr<Engine>> r;
    hipStream_t stream = nullptr;
    void** ptrs = nullptr;  // device [4][W]: xacc, res[0], res[1], partials of every rank
    GraphCache<int> graphs;  // by split count
    // 0: group_reduce_kernel; 1: the one-shot peer exchange's kernels (xchg.hip) -- every
    // rank's push, then every rank's reduce (one stream: the waits find their flags set);
    // 2: the producer-fused form -- every rank's o_proj / down / lm_head launch pushes from
    // its tail (tail_mode 1), then every rank's reduce kernel
    int xchg_mode = 0;

    ~Group();
    int init(const llmi_config& cfg, int world, int dev);
    int set_exchange(int mode);
    int reduce(int slot, int n, int op);
    int record_step(int nact);
    int decode(int n, int use_graph);
};

// Batched decode: n_seq sequence slots, each a whole single-rank Engine on ONE shared stream
// that borrows slot 0's weights (its own DecodeState, token / prompt buffers, KV cache,
// residual accumulators, q/k/v, activation, attention workspace and logits). A step over the
// active slots runs every slot's step_start, then per layer ONE multi-row GEMV (gemv_rows.hip)
// for q/k/v, the existing attention + o_proj launches per slot (that slot's own position and
// split count), ONE multi-row GEMV for gate_up and ONE for down, then ONE for the lm_head and
// each slot's sampler. The multi-row GEMV gives every row bitwise the single-row result, and
// everything else is the engine's own launch, so a slot's tokens and logits are bitwise those
// of an Engine decoding the sequence alone. W_o is still streamed once per slot. A slot's prompt
// can run through the engine's own (scored) prefill, one slot per call, on slot 0's prefill
// scratch, e4m3 weight copies and logits slab (Engine::pf_from): once per batch, not per slot.
struct Batch {
    std::vector<std::unique_ptr<Engine>> r;
    hipStream_t stream = nullptr;
    // captured steps by key {slot, nact, ...} of the active slots: what changes a step without
    // a setter call (a slot's setter drops the cache: Engine::invalidate)
    static constexpr size_t kMaxGraphs = 64;
    BatchGraphs graphs{kMaxGraphs};

    ~Batch();
    int init(const llmi_config& cfg, int n_seq, int dev);
    int slot_ok(int seq) const;
    int loaded();
    int reset(int seq);
    std::vector<int> active() const;
    int record_step(const std::vector<int>& act);
    int decode(int n, int use_graph);
    int prefill(int seq, int n, int split, bool scored);
    int fork(int src, const int* dst, int n_dst, int keep, const int32_t* ids, int n);  // engine_fork.hip
};

}  // namespace llmi

// ============================================================== C ABI handles
struct llmi_tp_comm {
    ncclComm_t c = nullptr;
};
struct llmi_engine {
    llmi::Engine e;
};
struct llmi_group {
    llmi::Group g;
};
struct llmi_batch {
    llmi::Batch b;
};
