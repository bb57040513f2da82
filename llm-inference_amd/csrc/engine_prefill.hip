// ------------------------------------------------------------ prefill
// Llama<T>::firstTokenGen (llama.cpp:273-316) / LlamaContextDecoder::forward
// (context_decoder.cpp:47-143): prompt rows [p0, p0 + n) in chunks of up to
// kPrefillRows through the MFMA GEMMs and the causal prefill attention, KV
// slots written; then the last row's final norm + lm_head + argmax, leaving
// the decode state exactly where n decode steps would have left it. The scored form also
// runs the final norm + lm_head GEMM over every chunk's rows and fills their logprob
// records. See engine.h.
#include "engine.h"

namespace llmi {

int Engine::alloc_prefill() {
    if (pf) return LLMI_OK;
    pf_rows = std::min(kPrefillRows, c.max_seq);
    const size_t R = pf_rows;
    Bump b;
    // qkv: two K slices of the gemm3 GEMM, summed by the rope kernel into slice 0
    const size_t ox = b.take(R * c.hidden * 4), oq = b.take(2 * R * (ql + 2 * kvrows) * 4), oo = b.take(R * ql * 4),
                 oa = b.take(R * il * 4);
    const size_t wide = std::max<size_t>(std::max<size_t>(c.hidden, ql), il);
    const size_t oh = b.take(R * wide * 2), ol = b.take(R * wide * 2), os = b.take(kPfSlabs * R * c.hidden * 4);
    // split-key attention partials: [heads][R / 64][8 chunks][64 x 128 + 128] fp32
    pf_split_floats = (size_t)hl * ((R + 63) / 64) * 8 * (64 * 128 + 128);
    const size_t osp = b.take(pf_split_floats * 4);
    LLMI_HIP(hipMalloc(&pf, b.off));
    pf_slab = (float*)(pf + os);
    pf_split = (float*)(pf + osp);
    pf_ah = (_Float16*)(pf + oh);
    pf_al = (_Float16*)(pf + ol);
    pf_x = (float*)(pf + ox);
    pf_qkv = (float*)(pf + oq);
    pf_o = (float*)(pf + oo);
    pf_act = (float*)(pf + oa);
    LLMI_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    return LLMI_OK;
}

// split mode 3 needs the fp8 lo pass of gemm3 on all four GEMMs (K multiples of 128)
bool Engine::lo8_supported() const {
    return wdt == LLMI_F16 && c.kv_dtype == LLMI_F16 && gemm3_supported(ql + 2 * kvrows, c.hidden, EPI_SLAB, 2) &&
           gemm3_supported(c.hidden, ql, EPI_SLAB, kPfDown) && gemm3_supported(2 * il, c.hidden, EPI_SILU_MUL, 1) &&
           gemm3_supported(c.hidden, il, EPI_SLAB, kPfDown) && c.hidden % 128 == 0 && ql % 128 == 0 &&
           il % 128 == 0 && ql / 128 >= kPfDown && il / 128 >= kPfDown;
}
int Engine::alloc_w8() {
    if (w8blob) return LLMI_OK;
    // e4m3 rows keep the fp16 row stride (2 K bytes, the first K used: gemm3.hip)
    const int H = c.hidden;
    const size_t nq = (size_t)(ql + 2 * kvrows) * H * 2, no = (size_t)H * ql * 2, ng = (size_t)2 * il * H * 2,
                 nd = (size_t)H * il * 2;
    Bump b;
    const size_t oq = b.take(nq), oo = b.take(no), og = b.take(ng), od = b.take(nd), per = b.off;
    LLMI_HIP(hipMalloc(&w8blob, per * layers.size()));
    w8l.assign(layers.size(), W8Layer{});
    for (size_t l = 0; l < layers.size(); ++l) {
        char* p = w8blob + l * per;
        W8Layer& w = w8l[l];
        w.qkv = p + oq;
        w.o = p + oo;
        w.gu = p + og;
        w.down = p + od;
        LLMI_TRY(w8_prepare(layers[l].qkv, ql + 2 * kvrows, H, w.qkv, &w.qkv_e, stream));
        LLMI_TRY(w8_prepare(layers[l].o, H, ql, w.o, &w.o_e, stream));
        LLMI_TRY(w8_prepare(layers[l].gu, 2 * il, H, w.gu, &w.gu_e, stream));
        LLMI_TRY(w8_prepare(layers[l].down, H, il, w.down, &w.down_e, stream));
    }
    LLMI_HIP(hipStreamSynchronize(stream));
    return LLMI_OK;
}

// rope + KV write + causal attention of rows [p0, p0 + m) of layer l: the fields both prefill
// paths share
PrefillAttnArgs Engine::prefill_attn_args(int l, int m, int p0) const {
    PrefillAttnArgs pa;
    pa.qkv = pf_qkv;
    pa.k_cache = kv_layer(l, 0);
    pa.v_cache = kv_layer(l, 1);
    pa.cache_dtype = c.kv_dtype; pa.max_seq = c.max_seq; pa.m = m; pa.p0 = p0;
    pa.k_scale = kv_scale_layer(l, 0); pa.v_scale = kv_scale_layer(l, 1);
    pa.heads = hl; pa.kv_heads = kvl; pa.head_dim = c.head_dim; pa.rope_tab = rope_tab; pa.out = pf_o;
    return pa;
}

// One prefill layer on the LDS-DMA GEMM (gemm2.hip): RMSNorm + split into fp16
// planes, q/k/v GEMM, rope + KV write + causal attention, split, o_proj (+residual),
// RMSNorm + split, gate_up GEMM writing silu(g) * u as planes, down (+residual).
int Engine::prefill_layer_gemm2(int l, int m, int p0, int split) {
    const Layer& L = layers[l];
    const int H = c.hidden;
    // split 3: the lo planes are e4m3 bytes against the e4m3 weight copies (gemm3.hip)
    const bool f8 = split == 3;
    const W8Layer* W8 = f8 ? &w8l[l] : nullptr;
    _Float16* lo = split >= 2 ? pf_al : nullptr;
    Gemm2Args g;
    g.a[0] = pf_ah; g.a[1] = lo; g.planes = split >= 2 ? 2 : 1; g.m = m; g.lo8 = f8 ? 1 : 0;
    // (previous down slices into x) + rmsnorm + qkv
    LLMI_TRY(rows_split_launch(pf_x, H, m, H, L.attn_norm, edt, c.rms_eps, pf_ah, lo, H, stream,
                               pf_pending ? pf_slab : nullptr, pf_pending, f8));
    pf_pending = 0;
    g.lda = H; g.w = L.qkv; g.n = ql + 2 * kvrows; g.k = H;
    g.ldy = g.n;
    if (f8) { g.w8 = W8->qkv; g.w8_exp = W8->qkv_e; }
    const bool qkv3 = gemm3_supported(g.n, H, EPI_SLAB, 2);
    if (qkv3) {  // two K slices (96 tiles alone would leave most CUs idle)
        g.epi = EPI_SLAB; g.ksplit = 2; g.slab = pf_qkv;
        LLMI_TRY(gemm3_launch(g, stream));
    } else {
        g.epi = EPI_STORE; g.y = pf_qkv;
        LLMI_TRY(gemm2_launch(g, stream));
    }
    // rope (+ the second qkv slice) + kv write + causal attention
    PrefillAttnArgs pa = prefill_attn_args(l, m, p0);
    pa.qkv2 = qkv3 ? pf_qkv + (size_t)m * g.n : nullptr;
    if (c.kv_dtype == LLMI_F16) {  // MFMA attention writes the o_proj input planes itself
        pa.mfma_planes = split >= 2 ? 2 : 1; pa.out_hi = pf_ah; pa.out_lo = lo; pa.out_lo8 = f8 ? 1 : 0;
        pa.split_ws = pf_split; pa.split_ws_floats = pf_split_floats;
    }
    LLMI_TRY(prefill_attn_launch(pa, stream));
    // o_proj + residual
    if (c.kv_dtype != LLMI_F16)
        LLMI_TRY(rows_split_launch(pf_o, ql, m, ql, nullptr, edt, 0.f, pf_ah, lo, ql, stream, nullptr, 0, f8));
    // split-K into slabs (128 tiles alone would leave half the CUs idle); the next
    // rows_split adds the slices into x in slice order (deterministic). The fp8 lo
    // pass is gemm3's: 8 slices of 256 x 256 tiles (256 workgroups)
    int so = (ql % (kPfSplit * 64)) == 0 ? kPfSplit : 1;
    g.lda = ql; g.w = L.o; g.w_kblock = 0; g.n = H; g.k = ql;
    g.epi = EPI_SLAB; g.ksplit = so; g.slab = pf_slab; g.y = pf_x; g.ldy = H;
    if (f8) {
        so = kPfDown; g.ksplit = so; g.w8 = W8->o; g.w8_exp = W8->o_e;
        LLMI_TRY(gemm3_launch(g, stream));
    } else {  // (the fp16 o_proj on gemm3's 8 K slices measured 0.1 ms slower a 7B prefill, r07l)
        LLMI_TRY(gemm2_launch(g, stream));
    }
    g.w_kblock = 0;
    // (o slices into x) + rmsnorm + gate_up + silu * up -> planes of the down GEMM's input
    LLMI_TRY(rows_split_launch(pf_x, H, m, H, L.ffn_norm, edt, c.rms_eps, pf_ah, lo, H, stream, pf_slab, so, f8));
    g.lda = H; g.w = L.gu; g.n = 2 * il; g.k = H;
    if (f8) {
        g.w8 = W8->gu; g.w8_exp = W8->gu_e;
        g.err = &st->error;
    }
    g.epi = EPI_SILU_MUL; g.pair_off = il; g.y = nullptr; g.y_hi = pf_act_h(); g.y_lo = split >= 2 ? pf_act_l() : nullptr;
    g.ldy = il;
    g.sk_slab = nullptr; g.sk_flags = nullptr; g.sk_grid = 0;
    // the whole K work of gate_up's 172 tiles spread evenly over every CU (gemm3 stream-K),
    // the fp8 lo pass included
    if (gemm3_supported(g.n, H, EPI_SILU_MUL, 1)) {
        g.err = &st->error;
        (void)gemm3_sk_attach(g, stream);
    }
    LLMI_TRY(gemm3_supported(g.n, H, EPI_SILU_MUL, 1) ? gemm3_launch(g, stream) : gemm2_launch(g, stream));
    // down + residual: K slices into slabs (gemm3: 8 uneven slices, 256 workgroups)
    g.sk_slab = nullptr; g.sk_flags = nullptr; g.sk_grid = 0;
    g.a[0] = pf_act_h(); g.a[1] = split >= 2 ? pf_act_l() : nullptr;
    g.lda = il; g.w = L.down; g.n = H; g.k = il;
    if (f8) { g.w8 = W8->down; g.w8_exp = W8->down_e; }
    g.epi = EPI_SLAB; g.pair_off = 0; g.y = pf_x; g.y_hi = g.y_lo = nullptr; g.ldy = H; g.slab = pf_slab;
    int sd;
    if (gemm3_supported(H, il, EPI_SLAB, kPfDown)) {
        sd = kPfDown; g.ksplit = sd;
        LLMI_TRY(gemm3_launch(g, stream));
    } else {
        sd = (il % (kPfSplit * 64)) == 0 ? kPfSplit : 1; g.ksplit = sd;
        LLMI_TRY(gemm2_launch(g, stream));
    }
    pf_pending = sd;  // added by the next layer's rows_split (or prefill_flush)
    return LLMI_OK;
}
int Engine::prefill_flush(int m) {  // pending down slices into x (after the last layer)
    if (!pf_pending) return LLMI_OK;
    LLMI_TRY(rows_split_launch(pf_x, c.hidden, m, c.hidden, nullptr, edt, 0.f, nullptr, nullptr, c.hidden, stream,
                               pf_slab, pf_pending));
    pf_pending = 0;
    return LLMI_OK;
}

// ------------------------------------------------------- scored prefill
// scored: after each chunk's layers, the final norm + an lm_head GEMM over the chunk's rows
// into the logits slab, then one logprob launch: row p writes record p + 1 with the scored
// id prompt[p + 1], every row but the call's last (whose record is rec_head's, as ever).
// Only the records, the activation planes and the slab are written.
int Engine::alloc_score() {
    if (sc_logits) return LLMI_OK;
    LLMI_HIP(hipMalloc(&sc_logits, (size_t)pf_rows * c.vocab * 4));
    return LLMI_OK;
}
// the scratch of this call: the engine's own, or -- a batch slot -- slot 0's, lent like the
// weights (one stream serialises its use). The e4m3 copies follow slot 0's weight reloads.
int Engine::prefill_scratch(int split, bool scored) {
    Engine& o = pf_from ? *pf_from : *this;
    LLMI_TRY(o.alloc_prefill());
    if (split == 3) LLMI_TRY(o.alloc_w8());
    if (scored) LLMI_TRY(o.alloc_score());
    if (&o == this) return LLMI_OK;
    pf = o.pf; pf_rows = o.pf_rows; pf_split_floats = o.pf_split_floats; n_cu = o.n_cu;
    pf_x = o.pf_x; pf_qkv = o.pf_qkv; pf_o = o.pf_o; pf_act = o.pf_act; pf_ah = o.pf_ah; pf_al = o.pf_al;
    pf_slab = o.pf_slab; pf_split = o.pf_split; sc_logits = o.sc_logits;
    if (split == 3) w8l = o.w8l; else w8l.clear();
    return LLMI_OK;
}
bool Engine::head_gemm_supported(bool use_gemm2) const {
    return use_gemm2 ? gemm2_supported(c.vocab, c.hidden, EPI_STORE)
                     : gemm_supported(edt, c.vocab, c.hidden, EPI_STORE);
}
// rows [p0, p0 + m) of pf_x (flushed): logits of all m rows, records of all but the call's last
int Engine::score_chunk(int m, int p0, int split, bool use_gemm2, bool last) {
    const int H = c.hidden;
    if (use_gemm2) {  // the path the layers took: planes, then the LDS-DMA GEMM (no e4m3 lm_head: two fp16 planes)
        _Float16* lo = split >= 2 ? pf_al : nullptr;
        LLMI_TRY(rows_split_launch(pf_x, H, m, H, final_norm, edt, c.rms_eps, pf_ah, lo, H, stream));
        Gemm2Args g;
        g.a[0] = pf_ah; g.a[1] = lo; g.planes = lo ? 2 : 1; g.lda = H; g.m = m;
        g.w = lm_head; g.n = c.vocab; g.k = H;
        g.epi = EPI_STORE; g.y = sc_logits; g.ldy = c.vocab;
        LLMI_TRY(gemm2_launch(g, stream));
    } else {  // the norm fused; int8 engines too (their lm_head is fp16)
        GemmArgs g;
        g.split = split == 1 ? 1 : 2;
        g.w_dtype = edt;
        g.m = m;
        g.a = pf_x; g.lda = H; g.gamma = final_norm; g.g_dtype = edt; g.eps = c.rms_eps;
        g.w = lm_head; g.n = c.vocab; g.k = H;
        g.epi = EPI_STORE; g.y = sc_logits; g.ldy = c.vocab;
        LLMI_TRY(gemm_launch(g, stream));
    }
    sc_p0 = p0;
    sc_m = m;
    const int rows = last ? m - 1 : m;
    if (rows == 0) return LLMI_OK;
    return engine_logprob_rows_launch(sc_logits, rows, c.vocab, prompt, p0 + 1, c.max_seq, lp_top, lp_tok(), lp_ids(),
                                      lp_tlp(), stream);
}
// test / debug read-back: the slab row of prompt position pos
int Engine::scored_logits_out(int pos, float* out, int n) {
    LLMI_REQUIRE(out && n >= 0 && n <= c.vocab, "scored_logits: bad arguments");
    LLMI_REQUIRE(sc_logits && sc_m > 0 && pos >= sc_p0 && pos < sc_p0 + sc_m,
                 "scored_logits: no scored chunk holds this position");
    LLMI_HIP(hipStreamSynchronize(stream));
    LLMI_HIP(hipMemcpy(out, sc_logits + (size_t)(pos - sc_p0) * c.vocab, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LLMI_OK;
}

int Engine::prefill(int n, int split, bool scored) {
    if (wdt == LLMI_I4) {
        set_last_error("[llmi][ERROR] prefill: int4 engines have no prefill GEMMs (run the prompt as decode steps)");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_REQUIRE(!grouped && c.tp_world == 1, "prefill: tensor-parallel prefill is not supported");
    LLMI_REQUIRE(prompt_len > 0, "prefill: set_prompt first");
    LLMI_REQUIRE(n >= 1 && host_next_pos + n <= prompt_len, "prefill: rows must lie inside the prompt");
    LLMI_REQUIRE(split >= 1 && split <= 3,
                 "prefill: split must be 1 (fp16 A), 2 (fp32-faithful) or 3 (fp16 hi + fp8 lo planes)");
    LLMI_REQUIRE(!scored || (lp_top >= 0 && lp_buf), "prefill_scored: set_logprobs first");
    if (!gemm_supported(wdt, ql + 2 * kvrows, c.hidden, EPI_STORE) || !gemm_supported(wdt, c.hidden, ql, EPI_ADD) ||
        !gemm_supported(wdt, 2 * il, c.hidden, EPI_SILU_MUL) || !gemm_supported(wdt, c.hidden, il, EPI_ADD))
        return decode(n, 1);  // fp32 weights / odd shapes: the decode kernels, one row at a time
    const bool use_gemm2 = wdt == LLMI_F16 && gemm2_supported(ql + 2 * kvrows, c.hidden, EPI_STORE) &&
                           gemm2_supported(c.hidden, ql, EPI_ADD) && gemm2_supported(2 * il, c.hidden, EPI_SILU_MUL) &&
                           gemm2_supported(c.hidden, il, EPI_ADD) && c.head_dim % 64 == 0;
    // no GEMM form for the lm_head shape: decode steps, which score every row themselves
    if (scored && !head_gemm_supported(use_gemm2)) return decode(n, 1);
    if (split == 3 && !(use_gemm2 && lo8_supported())) split = 2;  // shapes without the fp8 lo pass: exact planes
    LLMI_TRY(prefill_scratch(split, scored));
    const int H = c.hidden, p_begin = host_next_pos;
    for (int p0 = p_begin; p0 < p_begin + n; p0 += pf_rows) {
        const int m = std::min(pf_rows, p_begin + n - p0);
        LLMI_TRY(embedding_launch(prompt + p0, m, embed, edt, c.vocab, H, pf_x, stream));
        for (int l = 0; l < c.layers; ++l) {
            const Layer& L = layers[l];
            if (use_gemm2) {
                LLMI_TRY(prefill_layer_gemm2(l, m, p0, split));
                continue;
            }
            GemmArgs g;
            g.split = split == 3 ? 2 : split;
            g.w_dtype = wdt;
            g.m = m;
            // rmsnorm + qkv
            g.a = pf_x; g.lda = H; g.gamma = L.attn_norm; g.g_dtype = edt; g.eps = c.rms_eps;
            g.w = L.qkv; g.scales = L.qkv_s; g.n = ql + 2 * kvrows; g.k = H;
            g.epi = EPI_STORE; g.y = pf_qkv; g.ldy = g.n;
            LLMI_TRY(gemm_launch(g, stream));
            // rope + kv write + causal attention
            LLMI_TRY(prefill_attn_launch(prefill_attn_args(l, m, p0), stream));
            // o_proj + residual
            g.a = pf_o; g.lda = ql; g.gamma = nullptr;
            g.w = L.o; g.scales = L.o_s; g.n = H; g.k = ql;
            g.epi = EPI_ADD; g.y = pf_x; g.ldy = H;
            LLMI_TRY(gemm_launch(g, stream));
            g.w_kblock = 0;
            // rmsnorm + gate_up + silu * up
            g.a = pf_x; g.lda = H; g.gamma = L.ffn_norm;
            g.w = L.gu; g.scales = L.gu_s; g.n = 2 * il; g.k = H;
            g.epi = EPI_SILU_MUL; g.pair_off = il; g.y = pf_act; g.ldy = il;
            LLMI_TRY(gemm_launch(g, stream));
            // down + residual
            g.a = pf_act; g.lda = il; g.gamma = nullptr;
            g.w = L.down; g.scales = L.down_s; g.n = H; g.k = il;
            g.epi = EPI_ADD; g.pair_off = 0; g.y = pf_x; g.ldy = H;
            LLMI_TRY(gemm_launch(g, stream));
        }
        LLMI_TRY(prefill_flush(m));
        if (p0 + m == p_begin + n)  // last row -> x for the final norm + lm_head
            LLMI_HIP(hipMemcpyAsync(x, pf_x + (size_t)(m - 1) * H, (size_t)H * 4, hipMemcpyDeviceToDevice, stream));
        if (scored) LLMI_TRY(score_chunk(m, p0, split, use_gemm2, p0 + m == p_begin + n));
    }
    // the decode state first (cur_pos = last prompt row), then the head exactly as a
    // decode step runs it -- lm_head + argmax keys, and the top-K draw at step
    // seed + cur_pos + 1 when sampling (Llama<T>::firstTokenGen samples its token too)
    LLMI_TRY(prefill_finish_launch(st, prompt, tokens, p_begin, n, stream));
    LLMI_TRY(rec_head(true));
    host_next_pos += n;
    return LLMI_OK;
}

}  // namespace llmi
