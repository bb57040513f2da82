// Engine setup and teardown, the weight layout, and the three loaders (synthetic, the
// reference's fp32 files, W8A16 / W4A16 quantised on load). See engine.h.
#include "engine.h"
#include "prng.h"

namespace llmi {

Engine::~Engine() {  // teardown errors are not actionable; ignore them explicitly
    if (lp_buf) (void)hipFree(lp_buf);
    if (samp_ids) (void)hipFree(samp_ids);
    if (samp_vals) (void)hipFree(samp_vals);
    if (lr_bias) (void)hipFree(lr_bias);  // (lr_allowed is part of scratch)
    if (lr_out) (void)hipFree(lr_out);
    (void)graphs.drop(stream);  // the captured steps before the buffers their launches name
    (void)spec_graphs.drop(stream);
    lanes.clear();  // the verify lanes before what they borrow
    if (spec_draft) (void)hipFree(spec_draft);
    if (comm) (void)ncclCommDestroy(comm);
    for (void* p : peers_opened) (void)hipIpcCloseMemHandle(p);
    if (inbox) (void)hipFree(inbox);
    if (peers_dev) (void)hipFree(peers_dev);
    if (xchg_ep) (void)hipFree(xchg_ep);
    if (xt_cnt) (void)hipFree(xt_cnt);
    if (wblob) (void)hipFree(wblob);
    if (kcache && !kv_from) (void)hipFree(kcache);  // (a verify lane's cache is its engine's)
    if (vcache && !kv_from) (void)hipFree(vcache);
    if (scratch) (void)hipFree(scratch);
    if (!pf_from) {  // (a batch slot's are slot 0's)
        if (pf) (void)hipFree(pf);
        if (sc_logits) (void)hipFree(sc_logits);
    }
    if (w8blob) (void)hipFree(w8blob);
    if (rl_acc) (void)hipFree(rl_acc);
    if (rl_cnt) (void)hipFree(rl_cnt);
    if (wdt_blob) (void)hipFree(wdt_blob);
    if (qstage) (void)hipFree(qstage);
    if (stream && own_stream) (void)hipStreamDestroy(stream);
}

// ---------------------------------------------------------------- setup
// ext_stream != nullptr: rank of an in-process group (no RCCL communicator), or -- group_rank
// false -- a slot of a batch (struct Batch): a whole single-rank engine on the batch's stream.
// lender: the slot borrows that engine's weights (the Layer pointers are copied, nothing is
// allocated for them and nothing freed on destroy; the lender must outlive it)
int Engine::init(const llmi_config& cfg, int dev, const void* tp_id, hipStream_t ext_stream,
                 const Engine* lender, bool group_rank) {
    c = cfg;
    device = dev;
    const int W = c.tp_world;
    LLMI_REQUIRE(W >= 1 && c.tp_rank >= 0 && c.tp_rank < W, "engine: bad tp rank/world");
    LLMI_REQUIRE(c.head_dim == 128, "engine: head_dim must be 128");
    LLMI_REQUIRE(c.heads * c.head_dim == c.hidden, "engine: hidden != heads * head_dim");
    LLMI_REQUIRE(c.heads % c.kv_heads == 0, "engine: heads % kv_heads != 0");
    LLMI_REQUIRE(c.heads % W == 0 && c.kv_heads % W == 0 && c.inter % W == 0 && c.vocab % W == 0,
                 "engine: heads, kv_heads, inter and vocab must divide by tp_world");
    LLMI_REQUIRE(c.max_seq > 0 && c.layers > 0 && c.vocab > 0, "engine: bad dims");
    LLMI_REQUIRE(c.kv_dtype == LLMI_F16 || c.kv_dtype == LLMI_F32 || c.kv_dtype == LLMI_I8,
                 "engine: kv dtype must be f16, f32 or i8");
    wdt = c.weight_dtype;
    LLMI_REQUIRE(wdt == LLMI_F16 || wdt == LLMI_F32 || wdt == LLMI_I8 || wdt == LLMI_I4, "engine: bad weight dtype");
    if (wdt == LLMI_I4 && (W != 1 || ext_stream != nullptr)) {
        set_last_error("[llmi][ERROR] engine: int4 weights run on a single-rank engine only (tp_world 1, no "
                       "in-process group, no batch)");
        return LLMI_EUNSUPPORTED;
    }
    edt = (wdt == LLMI_F32) ? LLMI_F32 : LLMI_F16;
    wsz = dtype_size(wdt);  // (0 for int4: sizes go through row_bytes / lin_bytes)
    esz = dtype_size(edt);
    hl = c.heads / W;
    kvl = c.kv_heads / W;
    ql = hl * c.head_dim;
    kvrows = kvl * c.head_dim;
    il = c.inter / W;
    vl = c.vocab / W;
    if (wdt == LLMI_I4) {  // whole 128-column groups in q/k/v, gate_up and down; W_o is int8
        LLMI_REQUIRE(c.hidden % 128 == 0 && il % 128 == 0 && ql % 16 == 0,
                     "engine: int4 weights need hidden and inter in multiples of 128 (and q rows of 16)");
    } else {
        const int epl = 16 / (int)wsz;
        LLMI_REQUIRE(c.hidden % epl == 0 && ql % epl == 0 && il % epl == 0,
                     "engine: hidden, q rows per rank and inter per rank must be multiples of 16 bytes");
    }

    LLMI_HIP(hipSetDevice(device));
    LLMI_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (ext_stream) {
        stream = ext_stream;
        own_stream = false;
        grouped = group_rank;
    } else {
        LLMI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    // a communicator whenever an id is given -- also at tp_world 1, where the
    // all-reduces are identities but still run (captured in the token graph)
    // tp_world > 1 without an id: no RCCL; the ranks must open the one-shot peer
    // exchange (llmi_engine_xchg_open) before they decode
    if (!grouped && tp_id != nullptr) {
        ncclUniqueId id;
        std::memcpy(&id, tp_id, sizeof(id));
        ncclResult_t r = ncclCommInitRank(&comm, W, id, c.tp_rank);
        LLMI_REQUIRE(r == ncclSuccess, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    if (lender) {
        layers = lender->layers;
        embed = lender->embed;
        lm_head = lender->lm_head;
        final_norm = lender->final_norm;
        stream_bytes = lender->stream_bytes;
    } else {
        LLMI_TRY(alloc_weights());
    }
    LLMI_TRY(alloc_state());
    return LLMI_OK;
}

int Engine::alloc_weights() {
    const size_t H = c.hidden;
    Bump b;
    struct Off { size_t qkv, o, gu, down, qs, os, gs, ds, an, fn; };
    std::vector<Off> lo(c.layers);
    const size_t qkv_rows = ql + 2 * kvrows;
    for (int l = 0; l < c.layers; ++l) {
        Off& t = lo[l];
        t.qkv = b.take(lin_bytes(wdt, qkv_rows, H));
        t.o = b.take(lin_bytes(odt(), H, ql));
        t.gu = b.take(lin_bytes(wdt, 2 * il, H));
        t.down = b.take(lin_bytes(wdt, H, il));
        if (quantised()) {
            t.qs = b.take(scale_bytes(wdt, qkv_rows, H));
            t.os = b.take(scale_bytes(odt(), H, ql));
            t.gs = b.take(scale_bytes(wdt, 2 * il, H));
            t.ds = b.take(scale_bytes(wdt, H, il));
        }
        t.an = b.take(H * esz);
        t.fn = b.take(H * esz);
    }
    const size_t lm = b.take((size_t)vl * H * esz), fnorm = b.take(H * esz), emb = b.take((size_t)c.vocab * H * esz);
    wbytes = b.off;
    LLMI_HIP(hipMalloc(&wblob, wbytes));
    layers.resize(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        Layer& L = layers[l];
        L.qkv = wblob + lo[l].qkv;
        L.o = wblob + lo[l].o;
        L.gu = wblob + lo[l].gu;
        L.down = wblob + lo[l].down;
        if (quantised()) {
            L.qkv_s = (__half*)(wblob + lo[l].qs);
            L.o_s = (__half*)(wblob + lo[l].os);
            L.gu_s = (__half*)(wblob + lo[l].gs);
            L.down_s = (__half*)(wblob + lo[l].ds);
        }
        L.attn_norm = wblob + lo[l].an;
        L.ffn_norm = wblob + lo[l].fn;
    }
    lm_head = wblob + lm;
    final_norm = wblob + fnorm;
    embed = wblob + emb;
    // bytes streamed per forward: every linear weight (+scales), norms, lm_head, one embedding row
    // (int4: nibbles and group scales for q/k/v, gate_up and down; W_o int8 with its row scales)
    const uint64_t per_layer = lin_bytes(wdt, qkv_rows, H) + scale_bytes(wdt, qkv_rows, H) + lin_bytes(odt(), H, ql) +
                               scale_bytes(odt(), H, ql) + lin_bytes(wdt, 2 * il, H) + scale_bytes(wdt, 2 * il, H) +
                               lin_bytes(wdt, H, il) + scale_bytes(wdt, H, il) + 2 * H * esz;
    stream_bytes = per_layer * c.layers + (uint64_t)vl * H * esz + H * esz + H * esz;
    return LLMI_OK;
}

int Engine::alloc_state() {
    const size_t H = c.hidden;
    kv_layer_elems = (size_t)kvl * c.max_seq * c.head_dim;
    const size_t kvb = kv_alloc_bytes();  // int8: the rows, then their fp16 scales (zero: a zero row)
    if (kv_from) {  // a verify lane (engine_spec.hip): the engine's cache, nothing allocated
        kcache = kv_from->kcache;
        vcache = kv_from->vcache;
    } else {
        LLMI_HIP(hipMalloc(&kcache, kvb));
        LLMI_HIP(hipMalloc(&vcache, kvb));
        LLMI_HIP(hipMemsetAsync(kcache, 0, kvb, stream));
        LLMI_HIP(hipMemsetAsync(vcache, 0, kvb, stream));
    }
    if (kv_scale_bytes()) {
        kscale = reinterpret_cast<__half*>((char*)kcache + kv_align(kv_data_bytes()));
        vscale = reinterpret_cast<__half*>((char*)vcache + kv_align(kv_data_bytes()));
    }

    GemvArgs lmargs = lm_args();
    lm_grid = gemv_grid(lmargs);
    Bump b;
    const size_t o_ws = b.take(attn_workspace_bytes(hl, c.head_dim, c.max_seq));  // counters first
    const size_t o_st = b.take(sizeof(DecodeState));
    const size_t o_x = b.take(H * 4), o_qkv = b.take((ql + 2 * kvrows) * 4), o_att = b.take(ql * 4);
    const size_t o_xacc = b.take(H * 8), o_res0 = b.take(H * 8), o_res1 = b.take(H * 8);
    const size_t o_act = b.take((size_t)il * 4), o_log = b.take((size_t)vl * 4);
    const size_t o_par = b.take((size_t)lm_grid * 8);
    const size_t o_pr = b.take((size_t)c.max_seq * 4), o_tok = b.take((size_t)(c.max_seq + 1) * 4);
    const size_t o_rope = b.take((size_t)c.max_seq * c.head_dim * 4);
    const size_t o_qtag = b.take((size_t)(ql + 2 * kvrows) * 8);
    const size_t o_lra = b.take(lr_words() * 4);
    LLMI_HIP(hipMalloc(&scratch, b.off));
    LLMI_HIP(hipMemsetAsync(scratch, 0, b.off, stream));
    lr_allowed = (uint32_t*)(scratch + o_lra);  // the allowed bitmap of the logit rules: all ones = no mask
    LLMI_HIP(hipMemsetAsync(lr_allowed, 0xFF, lr_words() * 4, stream));
    attn_ws = scratch + o_ws;
    st = (DecodeState*)(scratch + o_st);
    x = (float*)(scratch + o_x);
    xacc = (long long*)(scratch + o_xacc);
    res[0] = (long long*)(scratch + o_res0);
    res[1] = (long long*)(scratch + o_res1);
    qkv_buf = (float*)(scratch + o_qkv);
    attn_out = (float*)(scratch + o_att);
    act = (float*)(scratch + o_act);
    logits = (float*)(scratch + o_log);
    partials = (unsigned long long*)(scratch + o_par);
    prompt = (int32_t*)(scratch + o_pr);
    tokens = (int32_t*)(scratch + o_tok);
    rope_tab = (float*)(scratch + o_rope);
    qtag = (unsigned long long*)(scratch + o_qtag);  // zeroed: tag 0 never matches (epochs start at 1)
    // cos/sin cache with HF's fp32 arithmetic (LlamaRotaryEmbedding._set_cos_sin_cache):
    // inv_freq = 1 / fp32(base ** (2i/d)) (torch's fp32 pow is correctly rounded),
    // angle = fp32(pos * inv_freq), cos/sin correctly rounded to fp32
    if (kv_from) {  // a verify lane reads the engine's table
        rope_tab = kv_from->rope_tab;
        LLMI_HIP(hipStreamSynchronize(stream));
        return LLMI_OK;
    }
    std::vector<float> tab((size_t)c.max_seq * c.head_dim);
    const int half = c.head_dim / 2;
    for (int i = 0; i < half; ++i) {
        const float p = (float)std::pow((double)c.rope_base, (double)(2 * i) / (double)c.head_dim);
        volatile float inv = 1.0f / p;
        for (int pos = 0; pos < c.max_seq; ++pos) {
            volatile float ang = (float)pos * inv;
            tab[((size_t)pos * half + i) * 2 + 0] = (float)std::cos((double)ang);
            tab[((size_t)pos * half + i) * 2 + 1] = (float)std::sin((double)ang);
        }
    }
    LLMI_HIP(hipMemcpyAsync(rope_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, stream));
    LLMI_HIP(hipStreamSynchronize(stream));
    return LLMI_OK;
}

// ----------------------------------------------------------- weights
// Every copy derived from the weights (the split-3 prefill's e4m3 copies) is dropped
// before any weight is written; it is rebuilt from the new weights on next use.
int Engine::weights_changed() {
    wdt_valid = false;  // the ring's W_down^T copies are rebuilt before the next ring decode
    if (w8blob) {
        LLMI_HIP(hipStreamSynchronize(stream));  // a prefill may still read them
        LLMI_HIP(hipFree(w8blob));
        w8blob = nullptr;
        w8l.clear();
    }
    return LLMI_OK;
}

int Engine::load_synthetic(uint64_t sd) {
    LLMI_TRY(weights_changed());
    seed = sd;
    if (wdt == LLMI_I4) return load_synthetic_i4();
    const int H = c.hidden, r = c.tp_rank;
    const int lin = (wdt == LLMI_I8) ? LLMI_SYN_INT8 : LLMI_SYN_LINEAR;
    auto fill = [&](void* dst, size_t row_off, int kind, int dt, uint32_t tid, int rows, int cols, int row0,
                    int col0, int ld) -> int {
        char* p = (char*)dst + row_off * (size_t)cols * dtype_size(dt);
        return synth_fill_launch(p, dt, kind, seed, tid, rows, cols, row0, col0, ld, stream);
    };
    for (int l = 0; l < c.layers; ++l) {
        Layer& L = layers[l];
        auto t = [&](uint32_t k) { return prng::layer_tid(l, k); };
        // fused [q; k; v] rows of this rank's heads (layer_weights.cc:25 order)
        LLMI_TRY(fill(L.qkv, 0, lin, wdt, t(prng::Q), ql, H, r * ql, 0, H));
        LLMI_TRY(fill(L.qkv, ql, lin, wdt, t(prng::K), kvrows, H, r * kvrows, 0, H));
        LLMI_TRY(fill(L.qkv, ql + kvrows, lin, wdt, t(prng::V), kvrows, H, r * kvrows, 0, H));
        // W_o row-major [H, ql] (a head-major layout measured no faster for the
        // split-by-head o_proj)
        LLMI_TRY(fill(L.o, 0, lin, wdt, t(prng::O), H, ql, 0, r * ql, c.heads * c.head_dim));
        // fused [gate; up] rows (layer_weights.cc:40 order)
        LLMI_TRY(fill(L.gu, 0, lin, wdt, t(prng::GATE), il, H, r * il, 0, H));
        LLMI_TRY(fill(L.gu, il, lin, wdt, t(prng::UP), il, H, r * il, 0, H));
        LLMI_TRY(fill(L.down, 0, lin, wdt, t(prng::DOWN), H, il, 0, r * il, c.inter));
        if (wdt == LLMI_I8) {
            const int S = LLMI_SYN_INT8_SCALE;
            LLMI_TRY(fill(L.qkv_s, 0, S, LLMI_F16, t(prng::Q), ql, 1, r * ql, 0, 1));
            LLMI_TRY(fill(L.qkv_s, ql, S, LLMI_F16, t(prng::K), kvrows, 1, r * kvrows, 0, 1));
            LLMI_TRY(fill(L.qkv_s, ql + kvrows, S, LLMI_F16, t(prng::V), kvrows, 1, r * kvrows, 0, 1));
            LLMI_TRY(fill(L.o_s, 0, S, LLMI_F16, t(prng::O), H, 1, 0, 0, 1));
            LLMI_TRY(fill(L.gu_s, 0, S, LLMI_F16, t(prng::GATE), il, 1, r * il, 0, 1));
            LLMI_TRY(fill(L.gu_s, il, S, LLMI_F16, t(prng::UP), il, 1, r * il, 0, 1));
            LLMI_TRY(fill(L.down_s, 0, S, LLMI_F16, t(prng::DOWN), H, 1, 0, 0, 1));
        }
        LLMI_TRY(fill(L.attn_norm, 0, LLMI_SYN_GAMMA, edt, t(prng::ATTN_NORM), 1, H, 0, 0, H));
        LLMI_TRY(fill(L.ffn_norm, 0, LLMI_SYN_GAMMA, edt, t(prng::FFN_NORM), 1, H, 0, 0, H));
    }
    LLMI_TRY(fill(lm_head, 0, LLMI_SYN_LINEAR, edt, prng::LM_HEAD, vl, H, r * vl, 0, H));
    LLMI_TRY(fill(final_norm, 0, LLMI_SYN_GAMMA, edt, prng::FINAL_NORM, 1, H, 0, 0, H));
    LLMI_TRY(fill(embed, 0, LLMI_SYN_EMBED, edt, prng::EMBED, c.vocab, H, 0, 0, H));
    LLMI_HIP(hipStreamSynchronize(stream));
    return LLMI_OK;
}

// int4: the quantisation of the fp16 engine's synthetic model. Every linear tensor is generated
// as fp32 (the fp16 values) into the staging buffer a block of rows at a time and quantised from
// there: q/k/v, gate_up and down in 4-bit groups, W_o to W8A16.
int Engine::load_synthetic_i4() {
    const int H = c.hidden;
    auto lin = [&](void* q, __half* sc, size_t row_off, int qdt, uint32_t tid, int rows, int cols) -> int {
        int chunk = 0;
        LLMI_TRY(quant_stage((size_t)cols * 4, rows, &chunk));
        float* rows_dev = reinterpret_cast<float*>(qstage + kQStageHead);
        for (int r0 = 0; r0 < rows; r0 += chunk) {
            const int n = std::min(chunk, rows - r0);
            LLMI_TRY(synth_fill_launch(rows_dev, LLMI_F32, LLMI_SYN_LINEAR, seed, tid, n, cols, r0, 0, cols, stream));
            LLMI_TRY(quant_rows(rows_dev, (size_t)cols, n, cols, q, sc, row_off + r0, qdt, nullptr));
        }
        return LLMI_OK;
    };
    auto fill = [&](void* dst, int kind, uint32_t tid, int rows, int cols) -> int {
        return synth_fill_launch(dst, edt, kind, seed, tid, rows, cols, 0, 0, cols, stream);
    };
    qstage_hold = true;
    int rc = LLMI_OK;
    for (int l = 0; l < c.layers && rc == LLMI_OK; ++l) {
        Layer& L = layers[l];
        auto t = [&](uint32_t k) { return prng::layer_tid(l, k); };
        auto run = [&]() -> int {
            LLMI_TRY(lin(L.qkv, L.qkv_s, 0, LLMI_I4, t(prng::Q), ql, H));
            LLMI_TRY(lin(L.qkv, L.qkv_s, ql, LLMI_I4, t(prng::K), kvrows, H));
            LLMI_TRY(lin(L.qkv, L.qkv_s, ql + kvrows, LLMI_I4, t(prng::V), kvrows, H));
            LLMI_TRY(lin(L.o, L.o_s, 0, LLMI_I8, t(prng::O), H, ql));
            LLMI_TRY(lin(L.gu, L.gu_s, 0, LLMI_I4, t(prng::GATE), il, H));
            LLMI_TRY(lin(L.gu, L.gu_s, il, LLMI_I4, t(prng::UP), il, H));
            LLMI_TRY(lin(L.down, L.down_s, 0, LLMI_I4, t(prng::DOWN), H, il));
            LLMI_TRY(fill(L.attn_norm, LLMI_SYN_GAMMA, t(prng::ATTN_NORM), 1, H));
            return fill(L.ffn_norm, LLMI_SYN_GAMMA, t(prng::FFN_NORM), 1, H);
        };
        rc = run();
    }
    if (rc == LLMI_OK) rc = fill(lm_head, LLMI_SYN_LINEAR, prng::LM_HEAD, vl, H);
    if (rc == LLMI_OK) rc = fill(final_norm, LLMI_SYN_GAMMA, prng::FINAL_NORM, 1, H);
    if (rc == LLMI_OK) rc = fill(embed, LLMI_SYN_EMBED, prng::EMBED, c.vocab, H);
    const hipError_t e = hipStreamSynchronize(stream);
    qstage_hold = false;
    quant_release();
    LLMI_TRY(rc);
    LLMI_HIP(e);
    return LLMI_OK;
}

// ------------------------------------------------ weights from the reference's files
// LlamaWeight<T>::loadWeights / LlamaLayerWeight<T>::loadWeights (llama_weights.cc:41-53,
// layer_weights.cc:48-66) with loadWeightFromBin<T, float> (weight_utils.cu:90-187): one
// raw fp32 file per (unsharded) tensor, fused qkv [(heads + 2 kv) * d, H] and gate_up
// [2 I, H]. The host converts to the engine's dtype (RNE, like the reference's
// fp32 -> half cast) and copies this rank's slice: q/k/v and gate/up rows, o/down
// columns, lm_head rows (the layout load_synthetic fills).
int Engine::put_host(void* dst, int dt, const float* src, size_t src_ld, int rows, int cols, size_t row0,
                     size_t col0, hipStream_t s) {
    const size_t n = (size_t)rows * cols, es = dtype_size(dt);
    std::vector<uint8_t> h(n * es);
    for (int r = 0; r < rows; ++r) {
        const float* a = src + (row0 + r) * src_ld + col0;
        if (dt == LLMI_F32) {
            std::memcpy(h.data() + (size_t)r * cols * 4, a, (size_t)cols * 4);
        } else {
            _Float16* o = reinterpret_cast<_Float16*>(h.data()) + (size_t)r * cols;
            for (int c2 = 0; c2 < cols; ++c2) o[c2] = (_Float16)a[c2];
        }
    }
    LLMI_HIP(hipMemcpyAsync(dst, h.data(), h.size(), hipMemcpyHostToDevice, s));
    LLMI_HIP(hipStreamSynchronize(s));  // h is released on return
    return LLMI_OK;
}

// W8A16 on load: rows [row0, row0 + rows) of the host fp32 tensor src [*, src_ld] go to the
// device staging buffer (whole rows, at most kQStageBytes at a time) and through the
// quantiser: q [rows, cols] = columns [col0, col0 + cols), the scale from the whole row.
void Engine::quant_release() {
    if (qstage) (void)hipFree(qstage);
    qstage = nullptr;
    qstage_bytes = 0;
}
// the staging buffer for blocks of at most *chunk rows of row_bytes each
int Engine::quant_stage(size_t row_bytes, int rows, int* chunk) {
    LLMI_REQUIRE(row_bytes <= kQStageBytes, "load_tensor: a row exceeds the quantiser's staging buffer");
    *chunk = (int)std::min<size_t>((size_t)rows, kQStageBytes / row_bytes);
    const size_t need = kQStageHead + (size_t)*chunk * row_bytes;
    if (need > qstage_bytes) {
        LLMI_HIP(hipStreamSynchronize(stream));
        quant_release();
        LLMI_HIP(hipMalloc(&qstage, need));
        qstage_bytes = need;
    }
    return LLMI_OK;
}
// n staged fp32 rows [n, ld] -> rows [q_row, q_row + n) of a quantised tensor of dtype qdt:
// LLMI_I8 the columns [col0, col0 + cols) with one scale a row, LLMI_I4 whole rows (col0 0,
// cols == ld) in 4-bit groups with cols / 128 scales a row
int Engine::quant_rows(const float* rows_dev, size_t ld, int n, int cols, void* q_dst, __half* s_dst, size_t q_row,
                       int qdt, int32_t* bad, int col0) {
    if (qdt == LLMI_I4) {
        LLMI_REQUIRE(col0 == 0 && (size_t)cols == ld, "load_tensor: int4 tensors are quantised in whole rows");
        return quantize_groups_i4_launch(rows_dev, ld, n, cols, static_cast<uint8_t*>(q_dst) + q_row * (size_t)(cols / 2),
                                         s_dst + q_row * (size_t)(cols / 128), bad, stream);
    }
    return quantize_rows_i8_launch(rows_dev, ld, n, (int)ld, col0, cols,
                                   static_cast<int8_t*>(q_dst) + q_row * (size_t)cols, s_dst + q_row, bad, stream);
}
int Engine::quant_put(const std::string& nm, const float* src, size_t src_ld, size_t row0, int rows, int col0,
                      int cols, void* q_dst, size_t q_row_off, __half* s_dst, int qdt) {
    const size_t row_bytes = src_ld * 4;
    int chunk = 0;
    LLMI_TRY(quant_stage(row_bytes, rows, &chunk));
    int32_t* bad = reinterpret_cast<int32_t*>(qstage);
    float* rows_dev = reinterpret_cast<float*>(qstage + kQStageHead);
    LLMI_HIP(hipMemsetAsync(bad, 0, 4, stream));
    for (int r0 = 0; r0 < rows; r0 += chunk) {
        const int n = std::min(chunk, rows - r0);
        LLMI_HIP(hipMemcpyAsync(rows_dev, src + (row0 + r0) * src_ld, (size_t)n * row_bytes, hipMemcpyHostToDevice,
                                stream));
        LLMI_TRY(quant_rows(rows_dev, src_ld, n, cols, q_dst, s_dst, q_row_off + r0, qdt, bad, col0));
    }
    int32_t nbad = 0;
    LLMI_HIP(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, stream));
    LLMI_HIP(hipStreamSynchronize(stream));
    if (nbad != 0) {
        set_last_error("[llmi][ERROR] load_tensor: " + nm + " holds a NaN or an infinity in " +
                       std::to_string(nbad) + " row(s); nothing usable was quantised from them");
        return LLMI_EINVAL;
    }
    return LLMI_OK;
}

// name: the reference's file stem without ".bin" (e.g. "model.layers.3.self_attn.qkv.weight")
// quantize (int8 and int4 engines only): the four linear tensors are quantised on the device, to
// W8A16, or -- int4 engines -- q/k/v, gate_up and down to 4-bit groups and o_proj to W8A16
int Engine::load_tensor(const char* name, const float* src, size_t count, bool quantize) {
    const int rc = load_tensor_impl(name, src, count, quantize);
    if (!qstage_hold) quant_release();
    return rc;
}

int Engine::load_tensor_impl(const char* name, const float* src, size_t count, bool quantize) {
    LLMI_REQUIRE(name && src, "load_tensor: null argument");
    LLMI_REQUIRE(!quantize || quantised(), "quantize needs an int8 engine (or an int4 one)");
    LLMI_TRY(weights_changed());
    const std::string nm(name);
    const size_t H = c.hidden, D = c.head_dim, QR = (size_t)c.heads * D, KR = (size_t)c.kv_heads * D;
    const size_t I = c.inter, r = c.tp_rank;
    auto need = [&](size_t n) -> int {
        if (count != n) {
            set_last_error("[llmi][ERROR] load_tensor: " + nm + " has " + std::to_string(count) + " values, expected " +
                      std::to_string(n));
            return LLMI_EINVAL;
        }
        return LLMI_OK;
    };
    auto lin_ok = [&]() -> int {
        LLMI_REQUIRE(quantize || !quantised(),
                     "load_tensor: int8 and int4 engines take fp32 weights only through the quantised loaders "
                     "(llmi_engine_load_bin_quantized / llmi_engine_load_tensor_quantized), or synthetic ones");
        return LLMI_OK;
    };
    if (nm == "model.embed_tokens.weight") {
        LLMI_TRY(need((size_t)c.vocab * H));
        return put_host(embed, edt, src, H, c.vocab, (int)H, 0, 0, stream);
    }
    if (nm == "lm_head.weight") {
        LLMI_TRY(need((size_t)c.vocab * H));
        return put_host(lm_head, edt, src, H, vl, (int)H, r * vl, 0, stream);
    }
    if (nm == "model.norm.weight") {
        LLMI_TRY(need(H));
        return put_host(final_norm, edt, src, H, 1, (int)H, 0, 0, stream);
    }
    const std::string pre = "model.layers.";
    LLMI_REQUIRE(nm.compare(0, pre.size(), pre) == 0, ("load_tensor: unknown tensor " + nm).c_str());
    size_t dot = nm.find('.', pre.size());
    LLMI_REQUIRE(dot != std::string::npos, ("load_tensor: unknown tensor " + nm).c_str());
    const int l = std::atoi(nm.substr(pre.size(), dot - pre.size()).c_str());
    LLMI_REQUIRE(l >= 0 && l < c.layers, ("load_tensor: layer out of range in " + nm).c_str());
    const std::string leaf = nm.substr(dot + 1);
    Layer& L = layers[l];
    const size_t ws = dtype_size(wdt);
    if (leaf == "input_layernorm.weight" || leaf == "post_attention_layernorm.weight") {
        LLMI_TRY(need(H));
        return put_host(leaf[0] == 'i' ? L.attn_norm : L.ffn_norm, edt, src, H, 1, (int)H, 0, 0, stream);
    }
    if (leaf == "self_attn.qkv.weight") {
        LLMI_TRY(lin_ok());
        LLMI_TRY(need((QR + 2 * KR) * H));
        if (quantize) {
            LLMI_TRY(quant_put(nm, src, H, r * ql, ql, 0, (int)H, L.qkv, 0, L.qkv_s, wdt));
            LLMI_TRY(quant_put(nm, src, H, QR + r * kvrows, kvrows, 0, (int)H, L.qkv, ql, L.qkv_s, wdt));
            return quant_put(nm, src, H, QR + KR + r * kvrows, kvrows, 0, (int)H, L.qkv, ql + kvrows, L.qkv_s, wdt);
        }
        char* d = (char*)L.qkv;
        LLMI_TRY(put_host(d, wdt, src, H, ql, (int)H, r * ql, 0, stream));
        LLMI_TRY(put_host(d + (size_t)ql * H * ws, wdt, src, H, kvrows, (int)H, QR + r * kvrows, 0, stream));
        return put_host(d + (size_t)(ql + kvrows) * H * ws, wdt, src, H, kvrows, (int)H, QR + KR + r * kvrows,
                        0, stream);
    }
    if (leaf == "self_attn.o_proj.weight") {
        LLMI_TRY(lin_ok());
        LLMI_TRY(need(H * QR));
        // column shard: every rank takes its scale from the whole unsharded row
        if (quantize) return quant_put(nm, src, QR, 0, (int)H, (int)(r * ql), ql, L.o, 0, L.o_s, odt());
        return put_host(L.o, wdt, src, QR, (int)H, ql, 0, r * ql, stream);
    }
    if (leaf == "mlp.gate_up_proj.weight") {
        LLMI_TRY(lin_ok());
        LLMI_TRY(need(2 * I * H));
        if (quantize) {
            LLMI_TRY(quant_put(nm, src, H, r * il, il, 0, (int)H, L.gu, 0, L.gu_s, wdt));
            return quant_put(nm, src, H, I + r * il, il, 0, (int)H, L.gu, il, L.gu_s, wdt);
        }
        LLMI_TRY(put_host(L.gu, wdt, src, H, il, (int)H, r * il, 0, stream));
        return put_host((char*)L.gu + (size_t)il * H * ws, wdt, src, H, il, (int)H, I + r * il, 0, stream);
    }
    if (leaf == "mlp.down_proj.weight") {
        LLMI_TRY(lin_ok());
        LLMI_TRY(need(H * I));
        if (quantize) return quant_put(nm, src, I, 0, (int)H, (int)(r * il), il, L.down, 0, L.down_s, wdt);
        return put_host(L.down, wdt, src, I, (int)H, il, 0, r * il, stream);
    }
    set_last_error("[llmi][ERROR] load_tensor: unknown tensor " + nm);
    return LLMI_EINVAL;
}

// Llama<T>::loadWeights(weight_path): weight_path + "<name>.bin" for every tensor.
int Engine::load_bin(const char* weight_path, bool quantize) {
    LLMI_REQUIRE(!quantize || quantised(), "quantize needs an int8 engine (or an int4 one)");
    qstage_hold = true;  // one staging buffer for all the tensors, released on return
    const int rc = load_bin_impl(weight_path, quantize);
    qstage_hold = false;
    quant_release();
    return rc;
}

int Engine::load_bin_impl(const char* weight_path, bool quantize) {
    LLMI_REQUIRE(weight_path, "load_bin: null path");
    std::vector<std::string> names = {"model.norm.weight", "lm_head.weight", "model.embed_tokens.weight"};
    for (int l = 0; l < c.layers; ++l)
        for (const char* leaf : {"input_layernorm.weight", "post_attention_layernorm.weight",
                                 "self_attn.qkv.weight", "self_attn.o_proj.weight", "mlp.gate_up_proj.weight",
                                 "mlp.down_proj.weight"})
            names.push_back("model.layers." + std::to_string(l) + "." + leaf);
    std::vector<float> buf;
    for (const std::string& nm : names) {
        const std::string path = std::string(weight_path) + nm + ".bin";
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) {
            set_last_error("[llmi][ERROR] load_bin: cannot open " + path);
            return LLMI_EINVAL;
        }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes < 0 || bytes % 4 != 0) {
            std::fclose(f);
            set_last_error("[llmi][ERROR] load_bin: " + path + " is not an fp32 file");
            return LLMI_EINVAL;
        }
        buf.resize((size_t)bytes / 4);
        const size_t got = std::fread(buf.data(), 4, buf.size(), f);
        std::fclose(f);
        if (got != buf.size()) {
            set_last_error("[llmi][ERROR] load_bin: short read on " + path);
            return LLMI_EINVAL;
        }
        LLMI_TRY(load_tensor_impl(nm.c_str(), buf.data(), buf.size(), quantize));
    }
    return LLMI_OK;
}
}  // namespace llmi
