/*
 * llmi.h -- C ABI of the MI355X-native Llama-2 decode engine (libllmi.so).
 *
 * This is the drop-in boundary for the reference's decode hot path
 * (Mr-wang27/llm-inference, the src/kernels launcher headers + the Llama<T> decode
 * loop). Every entry point is plain C: device pointers, sizes, dtype enums,
 * an opaque hipStream_t. No torch or C++ types cross it. Each function cites
 * the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - return 0 (LLMI_OK) on success, negative on error; never throws.
 *    LLMI_EINVAL = bad argument, LLMI_EUNSUPPORTED = valid but not built,
 *    LLMI_EHIP - hipError_t = HIP runtime error. llmi_last_error() returns a
 *    thread-local message "[llmi][ERROR] ..." (the reference's LLM_CHECK text
 *    convention, src/utils/macro.h:113-133).
 *  - Row-major tensors. Linear weights are [out_features, in_features]
 *    (PyTorch nn.Linear layout; every layer of the reference calls cuBLAS with
 *    trans_b on exactly this layout, src/kernels/linear.cu:38-99); the
 *    launcher's other forms (weight [in, out], a transposed input) are
 *    llmi_linear_trans.
 *  - Activations are fp32 unless a dtype argument says otherwise; weights
 *    may be fp32, fp16 or int8 (+ per-row fp16 scales, W8A16).
 *  - Nothing here blocks the host or allocates, except engine create/destroy and
 *    the engine's host<->device copy helpers; all launches are stream-ordered
 *    and graph-capturable.
 */
#ifndef LLMI_H_
#define LLMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* llmi_stream_t; /* hipStream_t; NULL = legacy default stream */

/* LLMI_I4: 4-bit group-quantised weights (W4A16; the format is stated at llmi_quantize_groups_i4) */
enum llmi_dtype { LLMI_F32 = 0, LLMI_F16 = 1, LLMI_I8 = 2, LLMI_I32 = 3, LLMI_I64 = 4, LLMI_I4 = 5 };

#define LLMI_OK 0
#define LLMI_EINVAL (-1)
#define LLMI_EUNSUPPORTED (-2)
#define LLMI_ENOMEM (-3)
#define LLMI_EHIP (-1000)

const char* llmi_last_error(void);
const char* llmi_version(void);

/* ======================================================================
 * Operator API: one entry per reference launcher on the decode path.
 * ==================================================================== */

/* launchInputEmbedding (src/kernels/input_embedding.h:6-9):
 * out[t, :] = table[ids[t], :] for t < n_tokens; out fp32 [n_tokens, hidden].
 * Bit-exact copy (fp16 -> fp32 widening is exact). ids out of range -> error flag. */
int llmi_embedding(const int32_t* ids, int n_tokens, const void* table, int table_dtype,
                   int vocab, int hidden, float* out, llmi_stream_t stream);

/* launchRMSNorm (src/kernels/rmsnorm_kernel.h:11-17):
 * out = gamma * (x * rsqrt(mean(x^2) + eps)) per row (modeling_llama.py:112-117).
 * residual_out (nullable) receives the pre-norm x (the reference's intent;
 * its kernel aliases it). x may alias out. */
int llmi_rmsnorm(const float* x, float* out, float* residual_out, const void* gamma, int gamma_dtype,
                 int n_tokens, int hidden, float eps, llmi_stream_t stream);

/* launchFusedAddBiasResidualRMSNorm (src/kernels/fused_addresidual_norm.h:9-15):
 * residual = residual + decoder_out (+ bias); decoder_out = rmsnorm(residual) * gamma.
 * bias is nullable (Llama-2 has none). */
int llmi_add_residual_rmsnorm(float* residual, float* decoder_out, const void* bias, int bias_dtype,
                              const void* gamma, int gamma_dtype, int n_tokens, int hidden, float eps,
                              llmi_stream_t stream);

/* launchAddResidual (src/kernels/add_residual.h:8-13): decoder_out += residual. */
int llmi_add_residual(const float* residual, float* decoder_out, int n_tokens, int hidden,
                      llmi_stream_t stream);

/* Elementwise f16 <-> f32 (round to nearest even): no reference counterpart; the
 * C++ mirror (include/llmi/kernels.h) stages TensorWrapper<half> activations of the
 * reference's fp16 instantiation through the fp32 operators with it. */
int llmi_convert(const void* src, int src_dtype, void* dst, int dst_dtype, size_t n, llmi_stream_t stream);

/* launchAct (src/kernels/act_kernel.h:8-9): in [n, 2, inter] (gate then up),
 * out[n, i] = silu(gate) * up. */
int llmi_silu_mul(const float* gate_up, float* out, int n_tokens, int inter, llmi_stream_t stream);

/* launchLinearGemm (src/kernels/linear.h:16-22) with trans_b = true:
 * y[m, n] = sum_k x[m, k] * W[n, k] (* scales[n] for int8). fp32 accumulate.
 * m = 1: the HBM-streaming GEMV. 2 <= m <= 8 (and larger m on shapes the GEMM tiles do not
 * cover, 8 rows at a time): the multi-row GEMV, which streams W once for the rows of a
 * launch; every row is bitwise the m = 1 result for that row. m > 8: batched (prefill) path. */
int llmi_linear(const float* x, const void* w, int w_dtype, const void* w_scales, float* y, int m,
                int n, int k, llmi_stream_t stream);

/* launchLinearGemm (src/kernels/linear.h:16-22, linear.cu:38-99) with both of its flags,
 * row-major: y[m, n] = op_a(x) . op_b(W), where
 *   op_a(x) = x [m, k]            (trans_a = 0)  or  x^T with x stored [k, m]  (trans_a = 1),
 *   op_b(W) = W stored [k, n]     (trans_b = 0, the reference's default: weight [in, out])
 *          or W^T with W [n, k]   (trans_b = 1: nn.Linear's [out, in], llmi_linear).
 * trans_b = 1, trans_a = 0 is llmi_linear itself; the other forms transpose the operand(s)
 * into a per-(device, stream) scratch (grown outside stream capture: run the shape once
 * before capturing) and then run llmi_linear, so every form has llmi_linear's arithmetic.
 * f16 / f32 weights; int8 weights only with trans_b = 1 (their scales are per output row).
 * Cost: trans_b = 0 transposes the WHOLE weight on every call (one extra n*k read and write,
 * so a weight-bound call moves ~3x the bytes of trans_b = 1); store weights [out, in] and pass
 * trans_b = 1 on a hot path, as every reference layer does. The scratch is kept per (device,
 * stream) for the process's lifetime, sized by the largest call. */
int llmi_linear_trans(const float* x, const void* w, int w_dtype, const void* w_scales, float* y, int m, int n, int k,
                      int trans_a, int trans_b, llmi_stream_t stream);

/* LLaMAFFNLayer::forward (ffn.cpp:52-93) for context rows as one call: y [m, hidden] =
 * W_down (silu(W_gate x) * (W_up x)), x [m, hidden] fp32, w_gate_up [2 inter, hidden] (gate
 * rows then up rows, the reference's fused gate_up_proj) and w_down [hidden, inter] fp16.
 * On the matrix cores with fp32-faithful split activations (llmi_linear's arithmetic); the
 * SiLU*up product goes from the gate_up epilogue straight into the down GEMM's input, never
 * to memory in fp32. LLMI_EUNSUPPORTED (nothing launched) for other dtypes / shapes: the
 * caller then runs llmi_linear + llmi_silu_mul + llmi_linear. */
int llmi_ffn(const float* x, const void* w_gate_up, const void* w_down, int w_dtype, float* y, int m, int hidden,
             int inter, llmi_stream_t stream);

/* The context decoder's projection + residual pair in one call (LlamaContextDecoder,
 * context_decoder.cpp:104-139): launchLinearGemm(o_proj) followed by
 * launchFusedAddBiasResidualRMSNorm (no bias), or the FFN followed by launchAddResidual and
 * the next layer's launchRMSNorm. With p = x . W^T (llmi_linear's arithmetic, K slices summed
 * in slice order): residual[m, n] += p, then out[m, n] = RMSNorm(residual) * gamma (gamma
 * null: out = residual; out null: the residual update alone). out may alias x (it is written
 * after x is read), not residual. fp16 weights, m >= 16, GEMM-tileable n / k, n <= 8192;
 * other cases return LLMI_EUNSUPPORTED with nothing launched (the caller runs the separate
 * launches). */
int llmi_linear_residual(const float* x, const void* w, int w_dtype, int m, int n, int k, float* residual, float* out,
                         const void* gamma, int gamma_dtype, float eps, llmi_stream_t stream);
/* llmi_ffn with the same residual epilogue: residual[m, hidden] += FFN(x), then out as above. */
int llmi_ffn_residual(const float* x, const void* w_gate_up, const void* w_down, int w_dtype, int m, int hidden,
                      int inter, float* residual, float* out, const void* gamma, int gamma_dtype, float eps,
                      llmi_stream_t stream);

/* Sticky device error bits recorded by launches on `stream` (current device) that have no
 * error word of their own -- llmi_linear / llmi_ffn / the *_residual calls: 16 = a stream-K
 * partial never arrived within 2 s (its workgroup could not run alongside the others), so
 * that output is incomplete. Synchronises the stream, stores the bits in *flags and clears
 * them. No counterpart in the reference (its cuBLAS calls have no cross-workgroup wait).
 * Concurrency: the stream-K control words (epoch, arrival count) live in a per-(device,
 * stream) workspace; launches on one workspace must not overlap, i.e. do not replay a graph
 * captured on stream S on another stream while eager stream-K launches run on S (the epoch
 * count would race silently). Launches on different streams use different workspaces. */
int llmi_stream_errors(llmi_stream_t stream, int* flags);

/* Test hook for the stream-K hand-off (no reference counterpart): the next `launches`
 * stream-K launches (any stream, this process) run with fault `mode` -- 1: no later piece
 * ever publishes its flag (every owner waiting on one times out after 2 s and sets bit 16),
 * 2: every later piece publishes 2.5 s late, after its owner gave up (a launch that follows
 * must still be correct: flags carry a per-launch epoch). 0 / launches 0 clears it. */
int llmi_debug_stream_k(int mode, int launches);

/* Test hooks for the decode engine's kernel forms (no reference counterpart; test-only: no
 * engine or operator path calls them). The operator calls above reach the GEMV only with an
 * fp32 x and the store / add / silu epilogues, and the decode attention only with its merge
 * kernel; a decoded token runs other forms of both. These hooks launch those forms directly.
 *
 * llmi_debug_gemv: every field is copied into the launcher's argument block as it stands and
 * the GEMV is launched once on `stream`. Zero (NULL) means "not used"; the only defaults are
 * eps 0 -> 1e-5 and ksplit 0 -> 1. w_dtype / g_dtype are llmi_dtype values. The caller owns
 * every buffer (device memory).
 *   w [n_rows, ldw (0: k)] with per-row fp16 `scales` for int8; w_dtype LLMI_I4: w [n_rows, k / 2]
 *   nibbles with `scales` fp16 [n_rows][k / 128] (llmi_quantize_groups_i4), k % 128 == 0, and only
 *   the forms of the token step: x_fixed + RMSNorm with epi 0 or 2, or an fp32 x with epi 4
 *   (ksplit 1); kpar > 1, ksplit > 1, ldw other than 0 or k, epi 1 and 3, an fp32 gamma and any
 *   other input form return LLMI_EUNSUPPORTED with nothing launched; x fp32 [k], or x_fixed int64
 *   [k] (value * 2^32) with RMSNorm, whose fp32 image workgroup 0 writes to x_out;
 *   gamma non-NULL: RMSNorm of x (gamma dtype g_dtype: f16 / f32) folded in;
 *   epi 0: y[r] = acc; 1: y[r] = acc + resid_scale * resid[r] (resid may alias y);
 *       2: y[g] = silu(acc[g]) * acc[g + pair_off] (n_rows = 2 pair_off);
 *       3: y[r] = acc, and workgroup b's best key (value bits << 32 | 0xFFFFFFFF - (idx_base + r))
 *          in partials[b];
 *       4: yacc[r] += fixed(acc) (int64, value * 2^32) with K split over ksplit workgroups; or,
 *          with yacc_single (ksplit 1), yacc[r] = yacc_base[r] (NULL: 0) + fixed(acc) stored,
 *          and the same value in yacc_copy[r] when given;
 *   grid > 0: that many workgroups (waves loop over row groups); kpar 2 / 4: K split over the
 *   waves of a workgroup (store / silu, RMSNorm, x_fixed, automatic grid);
 *   seed_dst non-NULL: seed_dst[0, seed_n) = seed_keep ? seed_src : 0 on the side.
 * llmi_debug_gemv_plan launches nothing: it checks the same arguments and reports the grid,
 * the unroll (16-B loads per row in flight: 4, 5 or 8) and the x-staging width (float4s of x
 * per thread: 4, 5, 11, 14, or 0 for the strided form) that llmi_debug_gemv will use. */
typedef struct llmi_debug_gemv_args {
    const void* w;
    const void* scales;
    int w_dtype, n_rows, k, ldw;
    const float* x;
    const long long* x_fixed;
    float* x_out;
    const void* gamma;
    int g_dtype;
    float eps;
    int epi;
    float* y;
    const float* resid;
    float resid_scale;
    int pair_off;
    unsigned long long* partials;
    uint32_t idx_base;
    int grid;
    int ksplit;
    long long* yacc;
    int yacc_single;
    const long long* yacc_base;
    long long* yacc_copy;
    const long long* seed_src;
    long long* seed_dst;
    int seed_n, seed_keep;
    int kpar;
} llmi_debug_gemv_args;
int llmi_debug_gemv(const llmi_debug_gemv_args* args, llmi_stream_t stream);
int llmi_debug_gemv_plan(const llmi_debug_gemv_args* args, int* grid, int* unroll, int* xpt);
/* llmi_debug_gemv_rows: the multi-row GEMV of a batched decode step -- args[0 .. m), 2 <= m <= 8,
 * are m activation rows against ONE weight matrix, streamed once. The blocks must agree in
 * every weight-side, shape and epilogue field (w, scales, w_dtype, n_rows, k, ldw, gamma,
 * g_dtype, eps, epi, resid_scale, pair_off, idx_base, grid, ksplit, yacc_single, seed_n,
 * seed_keep, kpar; else LLMI_EINVAL) and differ in the per-row pointers x / x_fixed, x_out, y,
 * resid, yacc, yacc_base, yacc_copy, partials, seed_src, seed_dst, which need not be
 * contiguous. Row i's outputs are bitwise those of llmi_debug_gemv(&args[i]). x is fp32
 * without RMSNorm (any epilogue) or x_fixed with RMSNorm (epi 0, 2, 3); other input forms and
 * kpar > 1 return LLMI_EUNSUPPORTED; m outside 2..8 LLMI_EINVAL. Nothing is launched on an error. */
int llmi_debug_gemv_rows(const llmi_debug_gemv_args* args, int m, llmi_stream_t stream);

/* llmi_debug_attn_oproj: one layer's decode attention as the engine's separate launches run
 * it -- the split-KV attention leaving its partials in `workspace` (no merge kernel), then the
 * o_proj that merges them by head and adds W_o . o into xacc[n_rows] (int64, value * 2^32)
 * with fixed-point atomics. The attention launch first seeds xacc: resid_scale 0 -> zeros,
 * else resid_fixed (int64) when given, else fixed(resid). Position: the device int *pos_dev;
 * nact > 0 must be *pos_dev / 64 + 1 (the grid holds only the active splits; a mismatch sets
 * bit 4 in *err and computes nothing), nact 0 sizes the grid for max_seq. k_cache / v_cache:
 * one layer [kv_heads, max_seq, head_dim] of cache_dtype; slot *pos_dev is written. w: W_o
 * [n_rows, ldw] (ldw >= heads * head_dim: a column shard of a wider matrix), or head_major
 * [heads][n_rows][head_dim]; per-row fp16 `scales` for int8. head_dim 0 -> 128, rope_base
 * 0 -> 10000. The caller owns every buffer, `workspace` (llmi_attn_workspace_bytes) included. */
typedef struct llmi_debug_attn_oproj_args {
    const float* qkv;
    void* k_cache;
    void* v_cache;
    int cache_dtype, max_seq;
    const int* pos_dev;
    int nact;
    int heads, kv_heads, head_dim;
    int rope;
    float rope_base;
    void* workspace;
    long long* xacc;
    const float* resid;
    const long long* resid_fixed;
    float resid_scale;
    const void* w;
    const void* scales;
    int w_dtype, head_major, n_rows, ldw;
    int* err;
    void* k_scale; /* cache_dtype LLMI_I8 (KV8): the layer's fp16 row scales [kv_heads, max_seq]; */
    void* v_scale; /* NULL: unused (an f16 / f32 cache) */
} llmi_debug_attn_oproj_args;
int llmi_debug_attn_oproj(const llmi_debug_attn_oproj_args* args, llmi_stream_t stream);
/* llmi_debug_attn_oproj_rows: the multi-row attention + o_proj of a speculative verify step --
 * args[0 .. m), 2 <= m <= 8, are m query rows of ONE sequence at consecutive positions
 * *args[0].pos_dev + i (the other blocks' pos_dev is not read) against ONE cache and ONE W_o:
 * one attention launch that loads every cached K / V row once and one o_proj launch that loads
 * W_o once. Row i sees keys 0 .. p + i; positions p .. p + m - 1 are written to the cache by
 * this call and never read from it. The blocks must agree in k_cache, v_cache, cache_dtype,
 * max_seq, heads, kv_heads, head_dim, rope, rope_base, w, scales, w_dtype, head_major, n_rows,
 * ldw, nact and err (else LLMI_EINVAL) and differ in qkv, workspace, xacc, resid, resid_fixed
 * and resid_scale; a row with neither resid nor resid_fixed is pre-seeded (its xacc is added
 * onto as it stands, the engine's form when the down GEMV wrote the seed). nact > 0 must be (*pos_dev + m - 1) / 64 + 1 (a mismatch sets bit 4 in *err
 * and computes nothing); nact 0 sizes the grid for max_seq. Row i's xacc, partials and cache
 * row are bitwise those of llmi_debug_attn_oproj(&args[i]) at position p + i, the rows run in
 * order. m outside 2..8: LLMI_EINVAL; an int8 cache: LLMI_EUNSUPPORTED. Nothing is launched on
 * an error. */
int llmi_debug_attn_oproj_rows(const llmi_debug_attn_oproj_args* args, int m, llmi_stream_t stream);

/* Diagnostics (no reference counterpart): while `stamps` (device memory, 8 u64 per
 * workgroup) is non-null, every launch of the transposed prefill attention kernel writes its
 * per-workgroup timeline there (WgStamp: start, copies of the first block landed, loop end,
 * end, __smid(), then query block | head << 16, key blocks). Null turns it off. */
int llmi_debug_prefill_stamps(void* stamps);

/* Test hooks for the prefill path's own kernels (no reference counterpart; test-only: no
 * engine or operator path calls them). llmi_engine_prefill is the only other way to these
 * kernels, and it fixes their shapes and chunking.
 *
 * llmi_debug_prefill_attn: one launch of the prefill attention -- rope + cache write of rows
 * [p0, p0 + m), then causal attention of those rows over cache slots [0, p0 + row] -- with
 * the launcher's argument block filled field for field (zero / NULL: not used; head_dim 0 ->
 * 128). qkv [m, (heads + 2 kv_heads) * 128] fp32, q rotated in place; qkv2: optional second
 * summand of the same layout; k_cache / v_cache: one layer [kv_heads, max_seq, 128] of
 * cache_dtype (f16 / f32); rope_tab [max_seq][64] (cos, sin) fp32 pairs; out [m, heads * 128].
 * mfma_planes 0: the scalar kernel; 1 / 2 (fp16 cache): the MFMA kernel with that many fp16
 * planes, its output in `out` or, with out_hi (, out_lo), as fp16 planes [m, heads * 128]
 * (out_lo8: out_lo rows hold e4m3 bytes of lo * 2^12 in their first half). split_ws
 * (split_ws_floats fp32 elements): scratch for split-key partials; chunk_blocks > 0 with
 * split_ws: 64-key blocks per chunk instead of the automatic choice. The caller owns every buffer.
 * llmi_debug_prefill_attn_plan launches nothing: it runs the same argument checks and the
 * function the launcher takes its plan from, and reports the key blocks per chunk (cb), the
 * chunk slots per query block (maxc; 1: no partials), the attention kernel's workgroup count
 * and the merge kernel's slot count (0: no merge launch, else 2, 4 or 8). The scalar form
 * reports cb 0, maxc 1, merge_slots 0. */
typedef struct llmi_debug_prefill_attn_args {
    float* qkv;
    const float* qkv2;
    void* k_cache;
    void* v_cache;
    int cache_dtype, max_seq;
    int m, p0;
    int heads, kv_heads, head_dim;
    const float* rope_tab;
    float* out;
    int mfma_planes;
    void* out_hi;
    void* out_lo;
    int out_lo8;
    float* split_ws;
    size_t split_ws_floats;
    int chunk_blocks;
    void* k_scale; /* cache_dtype LLMI_I8 (KV8, the scalar kernel only): the layer's fp16 row scales */
    void* v_scale; /* [kv_heads, max_seq]; NULL: unused (an f16 / f32 cache) */
} llmi_debug_prefill_attn_args;
int llmi_debug_prefill_attn(const llmi_debug_prefill_attn_args* args, llmi_stream_t stream);
int llmi_debug_prefill_attn_plan(const llmi_debug_prefill_attn_args* args, int* cb, int* maxc, int* grid,
                                 int* merge_slots);

/* llmi_debug_gemm: one launch of a prefill GEMM, Y (op)= sum_p A_p W^T, with the launcher's
 * argument block (Gemm2Args) filled field for field and handed to the production launcher
 * (test-only: no engine or operator path calls it). kernel 2: gemm2 (64 / 128 x 128 tiles);
 * 3: gemm3 (256 x 256 tiles). a_hi (, a_lo): fp16 planes [m, lda], planes 1 or 2; w fp16 [n, k].
 * epi: 0 store, 1 add, 5 slab (y [m, ldy] fp32; slab [ksplit][m][ldy]: slice s holds the sum
 * over its K range alone), 2 gate_up (w = [gate; up] rows, n = 2 x inter, the pair offset is set
 * to n / 2: silu(gate) * up into y [m, ldy] fp32 or, with y_hi (, y_lo), as fp16 planes).
 * lo8 (gemm3, planes 2): a_lo rows of 2 lda bytes whose first lda bytes are e4m3(lo * 2^12),
 * against w8 (rows of 2 k bytes, the first k = e4m3(W * 2^w8_exp)); gate_up then writes y_lo in
 * the same byte format. stream_k 1 (gemm3): gemm3_sk_attach first, as the engine's gate_up does
 * -- stream-K where that function takes it, the plain kernel where it declines; err: the sticky
 * error word (NULL: the stream's own, llmi_stream_errors). Nothing is allocated or launched on
 * a refused call. The caller owns every buffer.
 * llmi_debug_gemm_plan launches and allocates nothing: it runs the launcher's argument checks
 * and the functions the launchers take their choices from, and reports the row tile (bm: 64 or
 * 128 for gemm2, 256 for gemm3), the workgroup count, and the stream-K slots per tile (sk_pmax;
 * 0: the plain kernel -- one plane without lo8, more than 3 slots, or no stream_k). */
typedef struct llmi_debug_gemm_args {
    int kernel;
    const void* a_hi;
    const void* a_lo;
    int planes, lda;
    const void* w;
    int m, n, k;
    int epi;
    float* y;
    void* y_hi;
    void* y_lo;
    int ldy;
    int ksplit;
    float* slab;
    int lo8;
    const void* w8;
    int w8_exp;
    int stream_k;
    int* err;
} llmi_debug_gemm_args;
int llmi_debug_gemm(const llmi_debug_gemm_args* args, llmi_stream_t stream);
int llmi_debug_gemm_plan(const llmi_debug_gemm_args* args, int* bm, int* grid, int* sk_pmax);

/* llmi_debug_gemm1: one launch of the first-generation prefill GEMM (gemm.hip, the GEMM of the
 * int8 engines), its argument block (GemmArgs) filled field for field and handed to the
 * production launcher (test-only: no engine or operator path calls it). a: fp32 [m, lda],
 * split into fp16 planes while it is staged (split 2: hi + lo; 1: hi alone); gamma (g_dtype
 * LLMI_F16 / LLMI_F32, [k]; NULL: none): the RMSNorm of each a row folded in, with eps.
 * w: [n, k] of w_dtype LLMI_F16, or LLMI_I8 with scales, one fp16 per row. epi: 0 store (with
 * or without gamma), 1 add (y += .., no gamma), 2 gate_up (with gamma; w = [gate; up] rows,
 * n = 2 x inter, the pair offset is set to n / 2: y [m, ldy] = silu(gate) * up). w_kblock is
 * not exposed and stays 0. Nothing is launched on a refused call. The caller owns every buffer.
 * llmi_debug_gemm1_plan launches and allocates nothing: it runs the launcher's argument checks
 * and reports the row tile (bm: 64 or 128) and the workgroup count. */
typedef struct llmi_debug_gemm1_args {
    const float* a;
    int lda;
    const void* gamma;
    int g_dtype;
    float eps;
    const void* w;
    int w_dtype;
    const void* scales;
    int m, n, k;
    int split;
    int epi;
    float* y;
    int ldy;
} llmi_debug_gemm1_args;
int llmi_debug_gemm1(const llmi_debug_gemm1_args* args, llmi_stream_t stream);
int llmi_debug_gemm1_plan(const llmi_debug_gemm1_args* args, int* bm, int* grid);

/* llmi_debug_rows_split: the prefill GEMMs' activation producer. Rows of x [m, ldx] (k used):
 * with slab [ksplit][m][k] (ldx == k) x += slice 0 + slice 1 + ... in that order, written
 * back; then optional RMSNorm (gamma [k] of g_dtype f16 / f32; NULL: none); then fp16 planes
 * hi = fp16(v), lo = fp16(v - hi) in rows of ldh elements (lo NULL: hi alone; lo8: the first
 * ldh bytes of each lo row hold e4m3(clamp((v - hi) * 2^12, +-448)) instead; hi NULL with a
 * slab: the combine alone). k a multiple of 4, at most 8192. */
int llmi_debug_rows_split(float* x, int ldx, int m, int k, const void* gamma, int g_dtype, float eps, void* hi,
                          void* lo, int ldh, const float* slab, int ksplit, int lo8, llmi_stream_t stream);

/* llmi_debug_w8_prepare: the fp8 weight copy of the prefill GEMMs. w16 fp16 [rows, cols]
 * (cols a multiple of 8, 16-B aligned) -> w8 rows of 2 cols bytes whose first cols bytes are
 * e4m3(clamp(W * 2^exp, +-448)), the rest untouched; *exp (host) = the largest e with
 * max |W| * 2^e <= 448, 0 when the maximum is zero or not finite (a NaN or an infinity in W;
 * a NaN element stays a NaN byte). Synchronises the stream. */
int llmi_debug_w8_prepare(const void* w16, int rows, int cols, void* w8, int* exp, llmi_stream_t stream);

/* One decode row through the HBM-streaming GEMV with its fused prologue/epilogue -- what
 * LlamaSelfDecoder::forward strings together for a token (self_decoder.cpp:59-81 fused):
 *   gamma != NULL: x is RMS-normalised and scaled by gamma (dtype gamma_dtype) first;
 *   epilogue 0: y[n] = W x;  1: y[n] = W x + resid[n] (resid may not alias y);
 *   2: W is [gate; up] (n = 2 inter rows), y[inter] = silu(W_gate x) * (W_up x).
 * fp32 x / y / resid, W f16, f32 or i8 (+ scales). */
int llmi_linear_fused(const float* x, const void* w, int w_dtype, const void* w_scales, float* y, int n, int k,
                      const void* gamma, int gamma_dtype, float eps, int epilogue, const float* resid,
                      llmi_stream_t stream);

/* launchRoPE (src/kernels/qkv_bias_and_RoPE.h:40-42) for one decode token:
 * rotates q (heads) and k (kv_heads) of the fused qkv row [ (h + 2kv) * d ]
 * in place at position `pos` (= step - 1), pairs (i, i + d/2),
 * theta_i = base^(-2i/d) (modeling_llama.py:123-156, 204-236). */
int llmi_rope_decode(float* qkv, int pos, int heads, int kv_heads, int head_dim, float base,
                     llmi_stream_t stream);

/* launchDecoderMaskedMHA (src/kernels/fused_decoder_self_attention.h:10-19):
 * writes k, v of the fused qkv row into the cache slot `pos` of `layer`
 * (cache [layers, kv_heads, max_seq, head_dim], dtype f16 or f32), then
 * out[h] = softmax(q_h . K^T / sqrt(d)) V over positions 0..pos (fp32
 * softmax, split-KV over workgroups, log-sum-exp merge in a second launch).
 * rope != 0 additionally applies RoPE to q/k first (the engine's fused form).
 * workspace: >= llmi_attn_workspace_bytes(...) bytes of device memory (split
 * partials; no initialisation needed). */
size_t llmi_attn_workspace_bytes(int heads, int head_dim, int max_seq);
int llmi_attn_decode(const float* qkv, void* k_cache, void* v_cache, int cache_dtype, int layer,
                     int max_seq, int pos, int heads, int kv_heads, int head_dim, int rope,
                     float rope_base, float* out, void* workspace, llmi_stream_t stream);

/* KV8: the int8 KV cache (no reference counterpart; cache_dtype / kv_dtype LLMI_I8).
 * A cached row x[128] in fp32 (K after RoPE, V as produced) is stored as 128 two's-complement
 * int8 and ONE fp16 scale, by the W8A16 rule of llmi_quantize_rows_i8 on the row:
 *   amax = max |x_i|
 *   s    = fp16_rne(amax / 127); an fp16 zero becomes bits 0x0001 (2^-24), an infinity 0x7BFF (65504)
 *   q_i  = clamp(rint(x_i / float(s)), -127, 127)
 * with the correctly rounded fp32 divisions and rint round-half-even. A row holding a NaN or an
 * infinity stores scale bits 0x7E00 (NaN) and q = 0, so attention over it yields NaN as it does
 * with an fp16 cache. A cached value is float(q) * float(s), exact in fp32.
 * Storage: k_cache / v_cache [layers, kv_heads, max_seq, 128] int8 (8-byte aligned);
 * k_scale / v_scale [layers, kv_heads, max_seq] fp16. Quantisation is fused into the cache write
 * (the decode attention and the prefill's rope + cache write), dequantisation into the
 * attention's dot products: score_j = s_k[j] * sum_i q_i k8[j][i], o = sum_j (p_j s_v[j]) v8[j].
 * llmi_attn_decode_q8 is llmi_attn_decode over such a cache: cache_dtype must be LLMI_I8, the
 * scale of slot `pos` is written beside its row. */
int llmi_attn_decode_q8(const float* qkv, void* k_cache, void* v_cache, int cache_dtype, int layer,
                        int max_seq, int pos, int heads, int kv_heads, int head_dim, int rope,
                        float rope_base, float* out, void* workspace, llmi_stream_t stream, void* k_scale,
                        void* v_scale);

/* Copy the first n_rows cached rows of a whole cache to other caches (no reference counterpart;
 * what llmi_batch_fork does to the rows): rows [0, n_rows) of every (layer, kv head) of src_k and
 * src_v [layers, kv_heads, max_seq, 128] of cache_dtype LLMI_F32, LLMI_F16 or LLMI_I8 go to
 * dst_k[i] / dst_v[i] of the same shape, i < n_dst, raw bytes. One launch (kv_copy_rows_kernel):
 * every source byte is read once and stored n_dst times. With LLMI_I8 the fp16 scales
 * [layers, kv_heads, max_seq] (src_k_scale / src_v_scale -> dst_k_scale[i] / dst_v_scale[i]) are
 * copied as well; with the other dtypes the scale arguments are ignored and may be null. dst_*
 * are HOST arrays of n_dst device pointers, read before the call returns. Rows at or after n_rows
 * and their scales are not written in any destination; the source is only read. Any max_seq is
 * taken. Stream-ordered, no synchronisation, capturable.
 *   LLMI_EINVAL, with nothing launched: n_dst outside 1..7, n_rows outside [0, max_seq],
 * head_dim != 128, another cache dtype, a null or not 16-byte aligned buffer, a destination that
 * is the source or appears twice, LLMI_I8 without scales. n_rows == 0 succeeds and launches
 * nothing. */
int llmi_kv_copy_rows(const void* src_k, const void* src_v, const void* src_k_scale, const void* src_v_scale,
                      void* const* dst_k, void* const* dst_v, void* const* dst_k_scale, void* const* dst_v_scale,
                      int n_dst, int cache_dtype, int layers, int kv_heads, int max_seq, int head_dim, int n_rows,
                      llmi_stream_t stream);

/* launchTopKforBeamSearch + launchSampling (src/kernels/topK.h:51-56,
 * sampling.h:12-18) as wired by Llama<T> (K = beamwidth = 1, llama.cpp:59):
 * greedy argmax over logits[n]; ties -> lowest index. out_id: device int32. */
int llmi_argmax(const float* logits, int n, int32_t* out_id, llmi_stream_t stream);

/* launchTopKforBeamSearch (src/kernels/topK.h:51-56, topK.cu:24-191): per row of
 * logits [rows, vocab] (f32/f16), the k largest values in descending order -> topk_ids
 * [rows, k] (device int32) and topk_vals [rows, k] (same dtype). Ties -> lower index
 * (the reference's tie order follows its CUB reduction tree). k in [1, 16]; the
 * reference fixes K = 5 (topK.cu:154). vocab < k pads with id -1, value 1e-20 (topK.h:15-20). */
int llmi_topk(const void* logits, int dtype, int rows, int vocab, int k, int32_t* topk_ids, void* topk_vals,
              llmi_stream_t stream);

/* launchSampling (src/kernels/sampling.h:12-18, sampling.cu:28-115): for each row not yet
 * finished, topk_vals <- exp(v - v[0]) in place, threshold u * sum, output_id = the first id
 * whose running subtraction reaches <= 0 (% vocab), seqlen += 1, is_finished = (id == end_id).
 * u in (0, 1] is the reference's draw, curand_uniform of curand_init(step, row, 0): cuRAND's
 * XORWOW restated (rows < 65536). is_finished: device uint8 (C++ bool). */
int llmi_sampling(const int32_t* topk_ids, void* topk_vals, int dtype, int rows, int k, int32_t* output_id,
                  int32_t* seqlen, uint8_t* is_finished, int step, int end_id, int vocab, llmi_stream_t stream);

/* Temperature / top-k / top-p (nucleus) / repetition-penalty sampling over whole rows of
 * logits [rows, vocab] (f32, not modified). No reference counterpart; the rule is specified
 * in DESIGN.md ("Nucleus sampler") and restated in tests/nucleus_ref.py:
 *   penalty (skipped at 1): for every distinct id of the row's history, z = z > 0 ? z / r : z * r;
 *   temperature (skipped at 1): z = z / T (both divisions correctly rounded fp32);
 *   order: value descending, ties to the lower id (llmi_argmax's order: top_k = 1 is llmi_argmax);
 *   integer weights w = rint(expf(z - max) * 2^32); C = the first top_k of the order (0: all);
 *   K = the shortest prefix of C whose weight is >= ceil(top_p * sum(C)) (top_p = 1: C);
 *   the id returned is the first id of K, in ASCENDING ID order, whose running weight reaches
 *   ceil(u * sum(K)), u = curand_uniform(curand_init(step, row, 0)) as in llmi_sampling.
 * The id-order walk differs from llmi_sampling's value-order float walk: from the same u the
 * two samplers do not choose the same token.
 * Non-finite logits: -inf has weight 0; NaN (after penalty and temperature) counts as -inf;
 * if the maximum is +inf, the +inf entries share the draw equally and every other id has weight
 * 0 (a row of only -inf / NaN draws uniformly over all ids). The id is always in [0, vocab).
 * history [rows, history_stride] device int32 with history_len[row] valid ids per row
 * (history_len NULL: no history). out_kept (nullable) receives |K|. rows <= 65536,
 * vocab <= 131072 (LLMI_EUNSUPPORTED above). LLMI_EINVAL: temperature <= 0, top_p outside
 * (0, 1], repetition_penalty <= 0, top_k < 0, null pointers, history ids outside [0, vocab)
 * (ids are read back and checked unless the stream is being captured; the kernel ignores
 * such ids). Graph-capturable; allocates nothing but the XORWOW jump table (rows > 1, once). */
int llmi_sample_nucleus(const float* logits, int rows, int vocab, const int32_t* history, int history_stride,
                        const int32_t* history_len /* [rows], NULL: none */, float repetition_penalty,
                        float temperature, int top_k, float top_p, uint64_t step, int32_t* out_id /* [rows] */,
                        int32_t* out_kept /* [rows], nullable */, llmi_stream_t stream);

/* Log-probabilities over whole rows of logits [rows, vocab] (f32, not modified). No reference
 * counterpart; the rule is specified in DESIGN.md ("Log-probabilities") and restated in
 * tests/logprob_ref.py. z is the RAW logit: no penalty and no temperature are applied, so the
 * result describes the model's distribution, not the one a sampler draws from.
 *   NaN counts as -inf; m = max z;
 *   integer weights w_i = rint((double)expf(z_i - m) * 2^32); an id whose value equals the
 *   maximum has w_i = 2^32 exactly and z_i - m := 0 (llmi_sample_nucleus's convention);
 *   S = sum w_i, an integer sum: exact, hence the same bits in any summation order;
 *   logprob_i = (float)(((double)z_i - (double)m) - log((double)S * 2^-32)), in double;
 *   logsumexp = (float)((double)m + log((double)S * 2^-32)).
 * If the maximum is +inf, the +inf entries get -log(their count) and every other id -inf; a row
 * of only -inf / NaN gets -log(vocab) everywhere.
 * out_lp[row] = the logprob of ids[row] (ids NULL: out_lp is not written). top_ids / top_lp
 * [rows, n_top] = the first n_top ids of llmi_argmax's order (value descending, ties to the
 * lower id) and their logprobs, n_top in 0..8; n_top > vocab pads with id -1 and logprob -inf.
 * out_lse (nullable) receives the row's logsumexp. rows <= 65536, vocab <= 131072
 * (LLMI_EUNSUPPORTED above). LLMI_EINVAL: null logits, ids without out_lp, n_top outside [0, 8]
 * or without top_ids / top_lp, an id outside [0, vocab) (ids are read back and checked unless the
 * stream is being captured; the kernel writes nothing for such an id). One launch, one
 * workgroup per row; graph-capturable; allocates nothing. */
int llmi_logprobs(const float* logits, int rows, int vocab, const int32_t* ids /* [rows], nullable */, int n_top,
                  float* out_lp /* [rows] */, int32_t* top_ids /* [rows, n_top] */, float* top_lp /* [rows, n_top] */,
                  float* out_lse /* [rows], nullable */, llmi_stream_t stream);

/* Logit rules over whole rows of logits [rows, vocab] (f32, not modified): an additive bias, the
 * presence and frequency penalties over a history of ids, and an allowed-token bitmap. No
 * reference counterpart; the rule is specified in DESIGN.md ("Logit rules") and restated in
 * tests/logit_rules_ref.py. For id i, in this order, every step one round-to-nearest fp32
 * operation with no contraction:
 *   1. v = z[i]; NaN counts as -inf (llmi_sample_nucleus's convention);
 *   2. bias (nullable dense row [vocab], shared by the rows): if bias[i] != 0, v = v + bias[i]
 *      (bias[i] finite, or -inf: a ban; a zero of either sign leaves v's bits alone);
 *   3. c = the occurrences of i in the row's history; if c > 0 and a penalty is non-zero:
 *      t = frequency * (float)c; t = presence + t; v = v - t (the OpenAI / vLLM rule);
 *      a NaN that steps 2 and 3 produce (+inf meeting -inf) counts as -inf;
 *   4. allowed (nullable bitmap): bit i & 31 of word i >> 5 clear -> v = -inf. allowed_stride is
 *      in words: 0 = one bitmap of (vocab + 31) / 32 words for all rows, else row r's bitmap
 *      starts at word r * allowed_stride (>= (vocab + 31) / 32). Bits at or above vocab are ignored.
 * out [rows, vocab] receives the processed rows (out must not be logits) and out_ids [rows] the
 * argmax of each processed row in llmi_argmax's order (value descending, ties to the lower id;
 * a row of only -inf gives id 0). With no bias, no bitmap and zero penalties the processed row
 * is bitwise the raw row, NaN aside. Every count is an integer and every id's value is
 * computed from its own inputs alone, so the result has the same bits in any launch.
 * history [rows, history_stride] device int32 with history_len[row] valid ids per row
 * (history_len NULL: no history). rows <= 65536; vocab <= 131072 and history_stride <= 65535
 * (LLMI_EUNSUPPORTED above: 16-bit counters). LLMI_EINVAL: null logits / out / out_ids, out ==
 * logits, a penalty that is not finite, a bad allowed_stride, history_len without a history, a
 * bias value that is NaN or +inf, history_len outside [0, history_stride], history ids outside
 * [0, vocab) (the last three are read back and checked unless the stream is being captured;
 * the kernel clamps the length and ignores such ids). One launch, one workgroup per row;
 * graph-capturable; allocates nothing. */
int llmi_process_logits(const float* logits, int rows, int vocab, const float* bias /* [vocab], nullable */,
                        const uint32_t* allowed /* nullable */, int allowed_stride, const int32_t* history,
                        int history_stride, const int32_t* history_len /* [rows], NULL: none */,
                        float presence_penalty, float frequency_penalty, float* out /* [rows, vocab] */,
                        int32_t* out_ids /* [rows] */, llmi_stream_t stream);

/* The draw llmi_sampling makes, computed on the host (no device work): the first
 * curand_uniform of curand_init(seed, subsequence, 0) -- cuRAND's XORWOW as restated in
 * csrc/xorwow.h (subsequence < 65536). For checking the restatement against a CPU oracle. */
int llmi_curand_uniform(uint64_t seed, uint32_t subsequence, float* out);

/* launchRepeatKVCache (src/kernels/repeat_kv.h, repeat_kv.cu:7-91): caches [layers, batch,
 * kv_heads, max_seq, d] -> k_dst/v_dst [batch, heads, max_k_len, d], query head h reading kv
 * head h / (heads / kv_heads), positions < context_length[b] only. */
int llmi_repeat_kv(const void* k_cache, const void* v_cache, int dtype, int layer, const int32_t* context_length,
                   int batch, int kv_heads, int max_seq, int heads, int max_k_len, int head_dim, void* k_dst,
                   void* v_dst, llmi_stream_t stream);

/* ---- context-phase (prefill) operators of the reference's unfused attention layer
 * (LLaMAContextAttentionLayer::forward, context_attention.cpp:108-161). The engine's
 * llmi_engine_prefill fuses them; these are the per-launcher equivalents. dtype is
 * LLMI_F32 or LLMI_F16 for every tensor of a call (fp32 arithmetic); integer arrays
 * are device int32. Layouts are the reference's. */

/* launchCalPaddingoffset (src/kernels/cal_paddingoffset.h, .cu:51-86): input_lengths
 * [batch] -> padding_offset [sum of lengths] (token i sits at padded position
 * i + padding_offset[i] of [batch, max_q_len]) and cum_seqlens [batch + 1]. Lengths must
 * be <= max_q_len (the reference does not check; not checked on the device either). */
int llmi_padding_offset(int32_t* padding_offset, int32_t* cum_seqlens, const int32_t* input_lengths, int batch,
                        int max_q_len, llmi_stream_t stream);

/* launchAddFusedQKVBiasTransposeAndRoPE (src/kernels/qkv_bias_and_RoPE.h:26-36,
 * .cu:49-144), Llama (no bias): qkv [num_tokens, (heads + 2 kv_heads) * d] ->
 * q [batch, heads, seq_len, d], k, v [batch, kv_heads, seq_len, d]; token i goes to
 * padded position i + padding_offset[i]; q and k are rotated at position
 * history_length[b] + s (s = the token's index in its sequence), pairs (i, i + d/2),
 * with llmi_rope_decode's angle arithmetic. Two deliberate differences from the
 * reference kernel (bugs there): v is written (the reference leaves v_buf unset) and
 * the position is per sequence (the reference adds the packed token index, which is
 * the same thing at batch 1). */
int llmi_rope_qkv_prefill(const void* qkv, void* q, void* k, void* v, int dtype, const int32_t* padding_offset,
                          const int32_t* history_length, int num_tokens, int batch, int seq_len, int heads,
                          int kv_heads, int head_dim, float rope_base, llmi_stream_t stream);

/* launchConcatKVCache (src/kernels/concat_past_kv.h:11-18, .cu:16-143): k_src, v_src
 * [batch, kv_heads, max_q_len, d] -> caches [layers, batch, kv_heads, max_seq, d] at
 * slots history_length[b] + t for t < cur_query_length[b] of layer `layer`. */
int llmi_kv_append(const void* k_src, const void* v_src, int dtype, int layer, const int32_t* cur_query_length,
                   const int32_t* history_length, int batch, int kv_heads, int max_q_len, int head_dim, int max_seq,
                   void* k_cache, void* v_cache, llmi_stream_t stream);

/* launchBuildCausalMasks (src/kernels/build_causal_mask.h:8-11, .cu:4-45): mask
 * [batch, max_q_len, max_k_len] = 1 where q < q_lens[b], k < k_lens[b] and
 * k <= q + k_lens[b] - q_lens[b], else 0. (The reference's :29 also requires
 * k >= k_lens[b] - q_lens[b], which hides every history key from the chunk's queries;
 * identical without history. DESIGN.md §4.) */
int llmi_causal_mask(void* mask, int dtype, const int32_t* q_lens, const int32_t* k_lens, int batch,
                     int max_q_len, int max_k_len, llmi_stream_t stream);

/* The attention core of LLaMAContextAttentionLayer::forward after the cache append
 * (context_attention.cpp:125-161: launchRepeatKVCache -> QK^T launchLinearStridedBatchGemm
 * -> launchScaleMaskAndSoftmax with llmi_causal_mask's mask -> PV GEMM ->
 * launchTransposeOutRemovePadding) as ONE fused launch: q [batch, heads, max_q_len, d]
 * (rotated, fp32), caches [layers, batch, kv_heads, max_seq, d] (dtype LLMI_F32 or
 * LLMI_F16) of layer `layer` already holding each sequence's history and this chunk;
 * sequence b's query s (< input_length[b]) attends to slots k <= history_length[b] + s;
 * softmax(scale * qk) normalised by 1 / (sum + 1e-6) as the reference; out [num_tokens,
 * heads, d] fp32 with the sequences packed in batch order (launchCalPaddingoffset's
 * packing). head_dim 128. */
int llmi_context_attention(const float* q, const void* k_cache, const void* v_cache, int cache_dtype, int layer,
                           const int32_t* history_length, const int32_t* input_length, int batch, int heads,
                           int kv_heads, int max_q_len, int max_seq, int head_dim, float scale, float* out,
                           llmi_stream_t stream);

/* The same core with the two launchers in front of it fused in (launchAddFusedQKVBiasTransposeAndRoPE
 * + launchConcatKVCache, context_attention.cpp:108-124): qkv [num_tokens, (heads + 2 kv_heads) d]
 * fp32 rows (padding_offset as llmi_padding_offset makes it) are rotated at position
 * history_length[b] + s (llmi_rope_qkv_prefill's arithmetic), q goes to q_scratch [batch,
 * heads, max_q_len, d] and k / v straight into the cache slots llmi_kv_append would write
 * (rounded to the cache dtype), then llmi_context_attention runs. */
int llmi_context_attention_qkv(const float* qkv, const int32_t* padding_offset, const int32_t* history_length,
                               const int32_t* input_length, int num_tokens, int batch, int max_q_len, int heads,
                               int kv_heads, int head_dim, float rope_base, void* k_cache, void* v_cache,
                               int cache_dtype, int layer, int max_seq, float scale, float* q_scratch, float* out,
                               llmi_stream_t stream);
/* llmi_context_attention_qkv preceded by its q/k/v projection (context_attention.cpp:99's
 * launchLinearGemm): qkv = x [num_tokens, hidden] . w_qkv^T ((heads + 2 kv_heads) * head_dim
 * rows, fp16) with llmi_linear's arithmetic, its K slices summed in slice order by the RoPE
 * kernel as it reads them (the same values, no [num_tokens, qkv] pass). LLMI_EUNSUPPORTED
 * (nothing launched) for other weight dtypes / shapes: the caller runs llmi_linear first. */
int llmi_context_attention_proj(const float* x, const void* w_qkv, int w_dtype, int hidden,
                                const int32_t* padding_offset, const int32_t* history_length,
                                const int32_t* input_length, int num_tokens, int batch, int max_q_len, int heads,
                                int kv_heads, int head_dim, float rope_base, void* k_cache, void* v_cache,
                                int cache_dtype, int layer, int max_seq, float scale, float* q_scratch, float* out,
                                llmi_stream_t stream);

/* launchScaleMaskAndSoftmax (src/kernels/attn_softmax_kernel.h:8-12, .cu:79-174):
 * score[b, h, q, :] = softmax(scale * qk[b, h, q, :] + (1 - mask[b, q, :]) * -10000)
 * normalised by 1 / (sum + 1e-6) as the reference; qk, score [batch, heads, q_len,
 * k_len], mask [batch, q_len, k_len]. score may alias qk. */
int llmi_masked_softmax(const void* qk, const void* mask, void* score, int dtype, int batch, int heads, int q_len,
                        int k_len, float scale, llmi_stream_t stream);

/* launchLinearStridedBatchGemm (src/kernels/linear.h:29-36, .cu:126-229): for each of
 * `batch` matrices (contiguous, row-major) c[z] = op(a[z]) . op(b[z]); op(a) [m, k] is a
 * [m, k] or, with trans_a, a [k, m]; op(b) [k, n] is b [k, n] or, with trans_b, b [n, k];
 * c [m, n]; fp32 accumulate. QK^T: a = q, b = k, trans_b = 1; PV: a = scores, b = v. */
int llmi_batched_matmul(const void* a, const void* b, void* c, int dtype, int batch, int m, int n, int k, int trans_a,
                        int trans_b, llmi_stream_t stream);

/* launchTransposeOutRemovePadding (src/kernels/fused_transpose_and_remv_pad.h:7-9,
 * .cu:17-75): src [batch, heads, seq_len, d] -> dst [num_tokens, heads * d], token i
 * read from padded position i + padding_offset[i]. */
int llmi_transpose_remove_pad(const void* src, const int32_t* padding_offset, void* dst, int dtype, int num_tokens,
                              int batch, int seq_len, int heads, int head_dim, llmi_stream_t stream);

/* Synthetic-weight generator (replaces LlamaLayerWeight::loadWeights() dummy
 * path, src/weights/llama/layer_weights.cc:69-146). Fills the [rows, cols]
 * slice (row0, col0) of a logical [*, ld] tensor `tid` with llmi-prng-v1
 * values (spec: oracle/prng.py). kind: 0 linear, 1 embedding, 2 norm gamma
 * (rows = 1), 3 int8 weight, 4 int8 per-row scale (cols = 1).
 * out_dtype: F16 or F32 (values identical), I8 for kind 3, F16 for kind 4. */
enum llmi_synth_kind { LLMI_SYN_LINEAR = 0, LLMI_SYN_EMBED = 1, LLMI_SYN_GAMMA = 2,
                       LLMI_SYN_INT8 = 3, LLMI_SYN_INT8_SCALE = 4 };
int llmi_synth_fill(void* out, int out_dtype, int kind, uint64_t seed, uint32_t tid, int rows,
                    int cols, int row0, int col0, int ld, llmi_stream_t stream);
/* Host (CPU) twin of llmi_synth_fill, for checking the generator without a GPU. */
int llmi_synth_fill_host(void* out, int out_dtype, int kind, uint64_t seed, uint32_t tid, int rows,
                         int cols, int row0, int col0, int ld);
/* W8A16 quantiser (quant.hip; definition in DESIGN.md, int8 section): fp32 w [rows, ld]
 * with row_len data columns -> int8 q [rows, cols] (dense) = the columns [col0, col0 + cols)
 * and one fp16 scale per row, w ~= q * s. Per row: amax over all row_len columns (not only
 * the written slice; [row_len, ld) is padding and never read), s = fp16_rne(amax / 127)
 * (fp16 zero -> 2^-24, overflow -> 65504), q = clamp(rint(w / s), -127, 127) with correctly
 * rounded fp32 divisions and round-half-even. A row holding a NaN or an infinity gets s = 0,
 * q = 0 and adds 1 to *bad_rows (device counter the caller zeroes; may be NULL). All
 * pointers are device pointers; ld, row_len, col0 and cols are multiples of 4 with
 * col0 + cols <= row_len <= ld; w 16-byte aligned, q 4-byte. */
int llmi_quantize_rows_i8(const float* w, size_t ld, int rows, int row_len, int col0, int cols, int8_t* q,
                          void* scales /* fp16[rows] */, int32_t* bad_rows, llmi_stream_t stream);
/* W4A16 quantiser (quant.hip): fp32 w [rows, ld] with row_len data columns, row_len % 128 == 0
 * -> nibbles q uint8 [rows, row_len / 2] and fp16 scales [rows][row_len / 128], w ~= q * s.
 * The format, which the int4 GEMV decodes:
 *   Groups: 128 consecutive columns of one row.
 *   Scales: one fp16 scale per (row, group), layout s [rows][k / 128], row-major, in a
 *     separate array.
 *   Values: q lies in [-7, 7] and is stored as the nibble q + 8, two nibbles per byte, the low
 *     nibble holding the even column; a 16-byte chunk is 32 consecutive columns and a row is
 *     k / 2 bytes. The quantiser never writes nibble 0; the kernel decodes nibble 0 as -8.
 *   Definition (bit-exact against a numpy restatement):
 *     amax = max |w| over the group;
 *     s = fp16_rne(fp32(amax / 7)), an fp16 zero becomes 2^-24, an overflow becomes 65504;
 *     q = clip(rint(fp32(w / fp32(s))), -7, 7), divisions correctly rounded fp32, rint
 *       round-half-even.
 *     A row holding a NaN or an infinity gets q = 0 (nibble 8) and s = 0 in every group, and
 *     counts once in *bad_rows (device counter the caller zeroes; may be NULL).
 * Whole rows only; [row_len, ld) is padding and never read. All pointers are device pointers;
 * row_len <= ld, ld a multiple of 4, w 16-byte aligned, q 4-byte, scales 2-byte. */
int llmi_quantize_groups_i4(const float* w, size_t ld, int rows, int row_len, uint8_t* q,
                            void* scales /* fp16[rows][row_len / 128] */, int32_t* bad_rows, llmi_stream_t stream);
/* Device memory for host-side callers that include no HIP headers (the C++
 * mirror in include/llmi/): hipMalloc / hipFree / hipMemcpy / hipDeviceSynchronize.
 * kind: 0 host->device, 1 device->host, 2 device->device. */
int llmi_device_alloc(void** ptr, size_t bytes);
int llmi_device_free(void* ptr);
int llmi_device_memset(void* ptr, int value, size_t bytes);
/* stream-ordered form (hipMemsetAsync): the layer classes' scratch on their stream */
int llmi_device_memset_async(void* ptr, int value, size_t bytes, llmi_stream_t stream);
int llmi_memcpy(void* dst, const void* src, size_t bytes, int kind);
int llmi_device_sync(void);

/* Measured HBM read peak (the roofline's second denominator, SURVEY.md §8d timing rules):
 * one-shot launches that each read `bytes` (rounded down to whole 32-KB pieces per
 * workgroup) with non-temporal 16-B loads, 8 in flight per lane, cycling through the regions
 * of a 2 GiB buffer so every launch streams from HBM (not the 256 MiB Infinity Cache), timed
 * with HIP events over `iters` launches for grids of 512 / 1024 / 2048 / 4096 workgroups; the
 * best grid's average microseconds per launch, its GB/s and the bytes one launch read. */
int llmi_hbm_read_bench(size_t bytes, int iters, float* us, float* gbps, size_t* bytes_read);

/* Synthetic prompt ids (bench config: 8 PRNG ids). Host only. */
int llmi_synth_prompt(uint64_t seed, int n, int vocab, int32_t* out);

/* ======================================================================
 * Engine API: the Llama<T> decode loop (src/models/llama/llama.cpp:318-349
 * continueTokenGen, :362-457 Response) with the per-layer sequence of
 * LlamaSelfDecoder::forward (src/layers/decoder/self_decoder.cpp:23-89).
 * One engine per GPU (per TP rank). The whole token step -- embedding,
 * L x {rmsnorm+QKV, rope+kv-write+attention, O+residual, rmsnorm+gate_up+silu,
 * down+residual}, final norm + lm_head + argmax -- is one hipGraph replay;
 * positions and token ids live in device memory, so no host sync per token.
 * ==================================================================== */
typedef struct llmi_config {
    int hidden, heads, kv_heads, head_dim, inter, layers, vocab, max_seq;
    float rms_eps, rope_base;
    int weight_dtype; /* LLMI_F16 (default), LLMI_F32 (reference Llama<float>), LLMI_I8 (W8A16),
                       * LLMI_I4 (W4A16: q/k/v, gate_up and down in 4-bit groups of 128, W_o W8A16;
                       * tp_world 1, hidden and inter multiples of 128; decode steps only: prefill,
                       * the ring layer, llmi_batch_create and llmi_group_create return
                       * LLMI_EUNSUPPORTED) */
    int kv_dtype;     /* LLMI_F16 (throughput), LLMI_F32 (parity) or LLMI_I8 (KV8: int8 rows with one
                       * fp16 scale per (layer, kv head, position) -- the format: llmi_attn_decode_q8;
                       * any weight dtype; half the fp16 cache's bytes + 1.6 %. The fused q/k/v +
                       * attention launch is not taken, and prefill runs the scalar attention the
                       * fp32 cache runs: the MFMA attention and exact = 0 / fp8-lo modes need fp16) */
    int tp_rank, tp_world;
} llmi_config;

typedef struct llmi_engine llmi_engine;

/* Fill `cfg` with a preset: "llama2-7b", "llama2-13b", "tiny". */
int llmi_config_preset(const char* name, llmi_config* cfg);

/* RCCL unique id (128 bytes) for tensor parallel: rank 0 creates it, the
 * launcher broadcasts it (any side channel), every rank passes it to create. */
int llmi_tp_unique_id(void* out128);

/* Tensor-parallel all-reduce for operator-level callers (the sum of the
 * row-parallel partials after o_proj and down, modeling_llama.py pretraining_tp
 * semantics; the reference has none). One communicator per rank over RCCL (xGMI):
 * llmi_tp_comm_create on `device` with the broadcast id; llmi_tp_allreduce sums `count`
 * elements of buf in place across the ranks on `stream` (dtype LLMI_F32, LLMI_F16,
 * LLMI_I32 or LLMI_I64 -- the engine reduces its int64 fixed-point residual, exact and
 * order-independent). The engine owns its own communicator (llmi_engine_create). */
typedef struct llmi_tp_comm llmi_tp_comm;
int llmi_tp_comm_create(const void* tp_id, int world, int rank, int device, llmi_tp_comm** out);
int llmi_tp_allreduce(llmi_tp_comm* comm, void* buf, size_t count, int dtype, llmi_stream_t stream);
int llmi_tp_comm_destroy(llmi_tp_comm* comm);

/* device: HIP device ordinal. tp_id: 128-byte RCCL id (llmi_tp_unique_id, broadcast
 * to every rank): the engine creates an RCCL communicator and the token graph all-reduces
 * over it (with tp_world == 1 too: identities). With tp_world > 1 and tp_id NULL there is
 * no RCCL communicator: the ranks must open the one-shot peer exchange (below) before
 * they decode. */
int llmi_engine_create(const llmi_config* cfg, int device, const void* tp_id, llmi_engine** out);
int llmi_engine_destroy(llmi_engine* e);
/* Llama<T>::loadWeightsFromDummy (src/models/llama/llama.h) with llmi-prng-v1 weights. */
int llmi_engine_load_synthetic(llmi_engine* e, uint64_t seed);
/* LlamaWeight<T>::loadWeights(weight_path) (llama_weights.cc:41-53, layer_weights.cc:48-66,
 * loadWeightFromBin weight_utils.cu:90-187): reads weight_path + "<name>.bin", raw fp32, for
 * model.embed_tokens.weight, lm_head.weight, model.norm.weight and per layer l
 * model.layers.<l>.{input_layernorm, post_attention_layernorm, self_attn.qkv, self_attn.o_proj,
 * mlp.gate_up_proj, mlp.down_proj}.weight (unsharded shapes; this rank's slice is taken).
 * fp32 -> fp16 is round-to-nearest-even. int8 engines are refused here (the reference has
 * no int8 format): they take the same files through llmi_engine_load_bin_quantized. */
int llmi_engine_load_bin(llmi_engine* e, const char* weight_path);
/* One tensor of the same set from a host fp32 buffer (name without ".bin"; count checked). */
int llmi_engine_load_tensor(llmi_engine* e, const char* name, const float* host, size_t count);
/* The same loaders for an LLMI_I8 engine (any other: LLMI_EINVAL, "quantize needs an int8
 * engine"): same names, counts and files. The four linear tensors are uploaded as fp32 (whole
 * rows, at most 256 MiB staged at a time, freed on return) and quantised to W8A16 by
 * llmi_quantize_rows_i8 into the engine's int8 weights and fp16 row scales; the column-sharded
 * o_proj and down take each scale from the whole unsharded row, so every TP rank holds the
 * same scales. Norms, lm_head and the embedding are loaded as by llmi_engine_load_bin (fp16).
 * A linear tensor holding a NaN or an infinity fails with a message naming it.
 * An LLMI_I4 engine takes the same calls: q/k/v, gate_up and down go through
 * llmi_quantize_groups_i4 (nibbles + fp16 group scales), o_proj through llmi_quantize_rows_i8. */
int llmi_engine_load_bin_quantized(llmi_engine* e, const char* weight_path);
int llmi_engine_load_tensor_quantized(llmi_engine* e, const char* name, const float* host, size_t count);
/* Llama<T>::Sampling (llama.cpp:245-262: launchTopKforBeamSearch + launchSampling) inside the
 * decode step: k in [1, 16] samples each generated token from the top k logits with
 * sampling.cu's rule, u = curand_uniform(curand_init(step, 0, 0)) (cuRAND XORWOW restated)
 * at step = seed + (tokens so far, the sampled token's position) (seed 0: the reference's step,
 * llama.cpp:405-423);
 * k = 0 restores greedy argmax (the default). Needs tp_world == 1. Applies to tokens chosen
 * by decode steps (a batched prefill's first token stays greedy). */
int llmi_engine_set_sampling(llmi_engine* e, int k, uint64_t seed);
/* llmi_sample_nucleus inside the token step (one launch after the lm_head, and after a
 * prefill's last row): history = the sequence's ids up to the current position, read from
 * the device decode state, step = seed + (the sampled token's position). top_k 0 = no limit,
 * top_p 1 = no nucleus cut, temperature 1 and repetition_penalty 1 = off. Same checks as
 * llmi_sample_nucleus; needs tp_world == 1 and is not available on a group rank. Replaces
 * llmi_engine_set_sampling's sampler, and that call (any k, 0 included) replaces this one. */
typedef struct llmi_sampling_params {
    int top_k;
    float top_p, temperature, repetition_penalty;
    uint64_t seed;
} llmi_sampling_params;
int llmi_engine_set_sampling_params(llmi_engine* e, const llmi_sampling_params* p);
/* llmi_logprobs inside the token step: one more launch after the lm_head and after the sampler
 * (and after a prefill's last row), in the eager and the captured step alike. n_top = -1: off
 * (the default; nothing is launched and the captured step is unchanged); 0: the chosen token's
 * logprob only; 1..8: also that many alternatives. The forward at position p writes record
 * p + 1: the logprob, under the RAW logits of that forward (llmi_logprobs' rule: no penalty,
 * no temperature, whatever sampler is set), of the token the sequence holds at p + 1 -- the
 * prompt's while inside the prompt, else the id the sampler (or the argmax) chose -- and the
 * top n_top ids of that row with their logprobs. Independent of the sampler and kept across
 * changes of it. llmi_engine_set_prompt marks every record "not computed" (logprob NaN, ids
 * -1); record 0 is never computed, and the prompt rows that ran through llmi_engine_prefill's
 * batched pass stay not computed: only that call's last row forms logits, and it is recorded
 * (llmi_engine_prefill_scored fills them; without it, scoring a text steps it with
 * llmi_engine_decode). Changing n_top discards the
 * records. Needs tp_world == 1 and no group rank (LLMI_EUNSUPPORTED: only a vocab shard of
 * the logits is present); vocab <= 131072. */
int llmi_engine_set_logprobs(llmi_engine* e, int n_top);
/* The first n records (tok_lp [n], top_ids / top_lp [n, n_top]; each nullable). *n_valid = the
 * records that exist (positions stepped + 1, record 0 included), *n_top = the setting. Syncs. */
int llmi_engine_logprobs(llmi_engine* e, float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid,
                         int* n_top);
/* llmi_process_logits inside the token step: one launch after the lm_head and before the
 * sampler (and after a prefill's last row), in the eager and the captured step alike. For
 * every id of the raw row, in llmi_process_logits' order and arithmetic: an additive bias (a
 * -inf bias bans the id), presence / frequency penalties over the ids generated so far --
 * the history is tokens[prompt_len .. current position], or tokens[0 .. current position]
 * with count_prompt = 1; ids that llmi_engine_edit forces count as prompt -- and the allowed
 * set of llmi_engine_set_allowed. The processed row goes to a second buffer (the raw logits
 * are never written); greedy decoding takes its argmax (value descending, ties to the lower
 * id), and a sampler set with llmi_engine_set_sampling / llmi_engine_set_sampling_params
 * samples from the processed row instead of the raw one. Logprobs stay those of the raw row.
 * bias_ids / bias_values [n_bias]: sparse pairs in host memory, read before the call returns
 * (n_bias = 0: no bias); ids in [0, vocab) without duplicates, values finite or -inf, the
 * penalties finite, count_prompt 0 or 1 (LLMI_EINVAL otherwise). Each call replaces the bias
 * and the penalties of the one before and leaves the allowed set alone; rules are on while a
 * bias, a non-zero penalty or an allowed set is present, and with all three absent the step
 * is exactly the step without this call. LLMI_EUNSUPPORTED, with the engine left as it was:
 * tp_world > 1 or a group rank (only a vocab shard is present), speculation on, the ring
 * decode mode, vocab > 131072, penalties with max_seq > 65535 (16-bit counters). With rules
 * on, llmi_engine_set_speculation (k > 0) and llmi_engine_set_decode_mode(1) are refused. */
int llmi_engine_set_logit_rules(llmi_engine* e, const int32_t* bias_ids, const float* bias_values, int n_bias,
                                float presence_penalty, float frequency_penalty, int count_prompt);
/* The allowed set of the rules: every id not in ids [n] (host memory, read before the call
 * returns; in [0, vocab), LLMI_EINVAL otherwise) gets -inf. n = 0 with null ids removes the
 * mask; an empty set is impossible (n = 0 with non-null ids: LLMI_EINVAL). Replacing the
 * contents of a set that is present keeps the captured steps (the bitmap is a fixed engine
 * buffer updated in stream order), so a caller may change it between replayed steps:
 * constrained choice, a grammar. Same refusals as llmi_engine_set_logit_rules. */
int llmi_engine_set_allowed(llmi_engine* e, const int32_t* ids, int n);
/* Remove bias, penalties and allowed set: rules are off. */
int llmi_engine_clear_logit_rules(llmi_engine* e);
/* The processed row of the last step (fp32 [vocab]; n must equal vocab). Syncs. LLMI_EINVAL
 * while rules are off. */
int llmi_engine_processed_logits(llmi_engine* e, float* out, int n);
/* Reset the sequence and stage a prompt (device copy). */
int llmi_engine_set_prompt(llmi_engine* e, const int32_t* ids, int n);
/* Run n forward steps (one token each). use_graph: replay the captured hipGraph. */
int llmi_engine_decode(llmi_engine* e, int n_steps, int use_graph);
/* Speculative decoding (no reference counterpart): verify up to 8 positions of ONE sequence in
 * one pass over the weights and the KV cache, exact -- whatever is kept is bitwise what greedy
 * llmi_engine_decode produces.
 *
 * llmi_engine_set_speculation: max_draft in [0, 7] (else LLMI_EINVAL); allocates max_draft
 * extra lanes on first use (each its own activations, residual accumulators, attention
 * workspace, logits and argmax partials; the KV cache, the RoPE table and the weights are the
 * engine's), none at 0. LLMI_EUNSUPPORTED with max_draft > 0 for tp_world > 1 and group ranks,
 * int4 weights (the multi-row GEMV has no int4 form), an int8 KV cache, the ring decode mode,
 * an active sampler (llmi_engine_set_sampling k > 0, llmi_engine_set_sampling_params) and
 * logprobs; and while max_draft > 0 those setters return LLMI_EUNSUPPORTED in turn. */
int llmi_engine_set_speculation(llmi_engine* e, int max_draft);
/* One verify step at p = the next position: the pending token (the argmax the last forward
 * left, as a decode step would pick it) at p and draft[i - 1] at p + i run through the model as
 * n_draft + 1 rows -- per layer one multi-row GEMV each for q/k/v, gate_up and down, ONE
 * multi-row attention launch and ONE multi-row o_proj launch, then one multi-row lm_head.
 * With g_i the argmax of row i (ties to the lowest id), a = the largest value with
 * draft[j] == g_j for all j < a is accepted on the device, and the engine is left exactly
 * where a + 1 llmi_engine_decode steps would have left it: next position p + a + 1, tokens
 * p .. p + a, and row a's argmax partials, logits and hidden state. Cache rows p + a + 1 ..
 * p + n_draft hold rejected k / v; nothing reads them before they are overwritten. The call
 * synchronises and reads a few bytes back; *n_accepted = a. n_draft 0 runs the plain step.
 * Needs the prompt consumed, 0 <= n_draft <= max_draft, draft ids inside the vocabulary and
 * p + n_draft + 1 <= max_seq (else LLMI_EINVAL, nothing changed). use_graph: replay graphs
 * captured per (n_draft + 1, split count of p + n_draft). */
int llmi_engine_verify(llmi_engine* e, const int32_t* draft, int n_draft, int use_graph, int* n_accepted);
/* Prompt-lookup drafting, on the host (no GPU, no engine): for g = ngram_max down to ngram_min
 * with g <= n - 1, the suffix ids[n - g .. n) is searched among the starts 0 <= s <= n - g - 1;
 * the first g with a match wins and the LARGEST matching s is taken; the draft is
 * ids[s + g .. min(n, s + g + max_draft)) (it may run into the suffix itself). No match:
 * *n_out = 0. out holds max_draft ids. LLMI_EINVAL: a null pointer, ngram_min < 1,
 * ngram_max < ngram_min, max_draft outside [0, 7], n < 0. */
int llmi_lookup_draft(const int32_t* ids, int n, int ngram_max, int ngram_min, int max_draft, int32_t* out,
                      int* n_out);
/* Greedy generation with prompt-lookup drafts: advances the engine by exactly n_steps positions
 * and ends in bitwise the state llmi_engine_decode(e, n_steps, .) ends in. Each round drafts
 * (llmi_lookup_draft) from the sequence so far plus the pending token, trims the draft to
 * min(max_draft, remaining - 1, max_seq - p - 1) and calls llmi_engine_verify. The host keeps
 * its own copy of the token history (one read of the tokens at the start, then the accepted
 * counts). Needs the prompt consumed and llmi_engine_set_speculation(>= max_draft). stats
 * (nullable): verify steps run, ids drafted, ids accepted; verify_steps + accepted = n_steps. */
typedef struct llmi_spec_stats {
    int verify_steps, drafted, accepted;
} llmi_spec_stats;
int llmi_engine_generate_lookup(llmi_engine* e, int n_steps, int max_draft, int ngram_max, int ngram_min,
                                int use_graph, llmi_spec_stats* stats);
/* Edit a sequence in place (no reference counterpart): keep a prefix, force what follows. With P
 * the engine's next position (positions 0 .. P - 1 consumed; a pending token for P exists once
 * the prompt is used up), llmi_engine_edit(e, keep, ids, n) leaves positions 0 .. keep - 1
 * consumed, forgets the old pending token and everything at or after keep, and makes positions
 * keep .. keep + n - 1 take ids as a prompt would: afterwards the next position is keep and the
 * prompt length keep + n, and llmi_engine_decode, llmi_engine_prefill (from keep),
 * llmi_engine_verify and the samplers go on from there -- bitwise as an engine that was given
 * the kept ids + ids as its prompt. It rewinds a continuation, appends a turn without feeding
 * the history again (keep = P, ids = the pending token, then the turn), and gives a draft engine
 * the token its target chose.
 *   Needs a prompt set, 0 <= keep <= P, n >= 0, keep + n <= max_seq, every id in [0, vocab), and
 * n >= 1 unless keep == P (keep == P with n == 0 does nothing, the pending token included); each
 * violation returns LLMI_EINVAL and changes nothing. Allowed wherever llmi_engine_set_prompt is,
 * speculating engines included (the lanes are not touched); the ring decode mode returns
 * LLMI_EUNSUPPORTED.
 *   One stream-ordered launch (seq_edit_kernel) writes the device positions, ids into the prompt
 * buffer and the logprob records; for n <= 8 the ids travel in the launch arguments and the call
 * neither copies nor synchronises, a longer list is copied first and the call synchronises (as
 * llmi_engine_set_prompt). Nothing is cleared: cache rows at or after keep are stale and are
 * overwritten before any attention reads them (as a verify step's rejected rows); the device
 * error word and the forward counter are left alone; the captured step graphs stay valid.
 * Logprob records q >= keep become "not computed" (NaN / id -1) and records below keep keep
 * their bits; record keep itself STAYS not computed, because the forward at keep - 1 that would
 * write it is not run again. The scored-prefill slab is forgotten (llmi_engine_scored_logits).
 *
 * llmi_engine_position: the next position and the prompt length as the host tracks them (each
 * nullable); no synchronisation. */
int llmi_engine_edit(llmi_engine* e, int keep, const int32_t* ids, int n);
int llmi_engine_position(llmi_engine* e, int* next_pos, int* prompt_len);
/* Greedy generation with a second engine as the proposer (draft-model speculative decoding):
 * advances `target` by exactly n_steps positions and leaves it in bitwise the state
 * llmi_engine_decode(target, n_steps, .) leaves it in -- tokens, logits, hidden state and cache
 * -- WHATEVER the draft proposes; only the number of verify steps depends on the draft.
 *   The target: as llmi_engine_generate_lookup (prompt consumed, max_draft <=
 * llmi_engine_set_speculation's, LLMI_EINVAL), and nothing llmi_engine_set_speculation refuses
 * may be active (LLMI_EUNSUPPORTED). The draft: any single-rank engine in decode mode 0 on the
 * same device with the same vocab and max_seq >= the target's, not the target itself
 * (LLMI_EINVAL); its shape, seed, weight dtype (int4 included), KV dtype (int8 included) and
 * sampler are free: it only ever runs plain token steps.
 *   Host loop. Catch-up: the target's sequence is read once (pending token included); the draft
 * keeps the longest prefix it has already consumed with the same ids (none for a draft without
 * a prompt), is edited to the rest (llmi_engine_edit) and runs all but the last forced position
 * -- through its prefill (fp32-faithful planes) when draft_prefill != 0, more than one row is
 * missing and it has one (not int4), as decode steps otherwise. A cycle at target position p:
 * k = min(max_draft, remaining - 1, max_seq - p - 1); the draft steps until it holds k ids
 * beyond p (k steps, plus one per forced id it has not consumed); its tokens p + 1 .. p + k are
 * read back (k ids and the draft's error word) and verified (llmi_engine_verify: a accepted,
 * next token g); the draft is edited to keep = min(p + a + 1, p + k) with the target's tokens
 * keep .. p + a + 1 -- one id, or two when every proposal was accepted -- which travel in the
 * launch arguments, so the draft adds one synchronisation a cycle (the read-back).
 * stats (nullable) as llmi_engine_generate_lookup. The draft is left aligned with the target:
 * a second call finds nothing to catch up. */
int llmi_engine_generate_draft(llmi_engine* target, llmi_engine* draft, int n_steps, int max_draft,
                               int draft_prefill, int use_graph, llmi_spec_stats* stats);
/* Prefill (Llama<T>::firstTokenGen, llama.cpp:273-316; LlamaContextDecoder::forward,
 * context_decoder.cpp:47-143): the next n_tokens prompt rows in one batched pass
 * (chunks of 512) -- MFMA GEMMs, causal prefill attention, KV slots written --
 * then the last row's lm_head + argmax. Afterwards the engine is exactly where
 * n_tokens decode steps would have left it, so llmi_engine_decode continues.
 * exact = 1: fp32-faithful GEMMs (activations split into two fp16 halves);
 * exact = 2: the fp16 hi half exact, the remainder as e4m3 against e4m3 weight
 *   copies on the block-scaled fp8 MFMA (~1e-4 relative; the copies are made on the
 *   first such call and kept at the fp16 row stride, i.e. as many bytes as the fp16
 *   GEMM weights; an fp32 KV cache or shapes without K % 128 == 0 fall back to
 *   exact = 1);
 * exact = 0: activations rounded to fp16 (faster, ~1e-3 relative at 32 layers).
 * Rows must lie inside the prompt; tp_world must be 1. fp32 weights run the
 * decode kernels row by row. */
int llmi_engine_prefill(llmi_engine* e, int n_tokens, int exact);
/* llmi_engine_prefill that also fills the log-probability records of the rows it consumes
 * (prompt "echo" logprobs, text scoring at prefill speed). Arguments, checks and effect are
 * llmi_engine_prefill's: tokens, the final logits, the decode state and the KV cache are
 * bitwise what that call leaves, and so is the record of the call's last row. In addition,
 * after each chunk's layers, the final RMSNorm and an lm_head GEMM over the chunk's rows
 * write fp32 logits into a slab [512][vocab] (allocated on the first scored call: 65.5 MB at
 * vocab 32000), and one launch of the logprob kernel lets every row p but the call's last
 * write record p + 1 with the scored id prompt[p + 1] -- llmi_logprobs' rule on the raw
 * logits. The head GEMM runs on the path the layers took (exact 1 and 2: two fp16 activation
 * planes -- there is no e4m3 copy of the lm_head; exact 0: one), so a record agrees with the
 * token step's to the GEMM's accuracy, not bitwise. Where no GEMM form takes the lm_head
 * shape (and for fp32 weights) the call runs as decode steps, which score every row.
 * LLMI_EINVAL when logprobs are off (llmi_engine_set_logprobs first); nothing is launched on
 * an error. */
int llmi_engine_prefill_scored(llmi_engine* e, int n_tokens, int exact);
/* Test / debug read-back: the first n fp32 logits of prompt position pos as the last scored
 * chunk's lm_head GEMM left them (the call's last row included). LLMI_EINVAL if that chunk
 * does not hold pos (llmi_engine_set_prompt forgets the chunk). Syncs. */
int llmi_engine_scored_logits(llmi_engine* e, int pos, float* out, int n);
/* Block until the engine stream is idle. */
int llmi_engine_sync(llmi_engine* e);
/* Tokens[0 .. n) of the sequence so far: prompt ids followed by generated ids
 * (position p's token; the token after the last forward is included). */
int llmi_engine_tokens(llmi_engine* e, int32_t* out, int n, int* n_valid);
/* fp32 logits of the last forward (this rank's vocab shard under TP). */
int llmi_engine_logits(llmi_engine* e, float* out, int n);
/* fp32 residual stream (hidden) after the last forward. */
int llmi_engine_hidden(llmi_engine* e, float* out, int n);
/* Read one cache slot (layer, pos) of K or V as fp32 [kv_heads_local, head_dim] (an int8
 * cache: the dequantised q * s). */
int llmi_engine_kv_slot(llmi_engine* e, int layer, int pos, int which_v, float* out);
/* An int8 cache's slot as stored: q [kv_heads_local, head_dim] int8 and the rows' fp16 scale
 * bits [kv_heads_local]. LLMI_EINVAL on an f16 / f32 cache. */
int llmi_engine_kv_slot_q8(llmi_engine* e, int layer, int pos, int which_v, int8_t* q, uint16_t* scale_bits);
/* Bytes of weights (and KV per position: K and V rows, with an int8 cache their scales too --
 * layers * kv_heads * (128 + 2) * 2) one forward streams on this rank. */
int llmi_engine_bytes(llmi_engine* e, uint64_t* weight_bytes, uint64_t* kv_bytes_per_pos);
/* hipStream_t the engine launches on. */
llmi_stream_t llmi_engine_stream(llmi_engine* e);
/* Time `iters` eager launches of one kernel (HIP events on the engine stream);
 * launch i runs layer i % layers, so its weights stream from HBM as in decode.
 * which: 0 qkv, 1 attn, 2 o, 3 gate_up, 4 down, 5 lm_head; 6 / 7 one TP residual
 * all-reduce (RCCL int64, hidden elements; engines created with a tp_id) launched
 * eagerly / replayed from one captured graph of `iters` calls -- a collective: every
 * rank must make the same call.
 * avg_us receives the mean duration; bytes the algorithmic bytes per launch. */
int llmi_engine_time_kernel(llmi_engine* e, int which, int iters, float* avg_us, uint64_t* bytes);
/* which 8 / 9: the same residual exchange over the one-shot peer path (below), eager /
 * graph-replayed -- also a collective. which 10: the persistent ring layer (decode mode 1,
 * below): o_proj + gate_up + down + the next layer's q/k/v in one launch. */

/* Decode structure of a token (no reference counterpart: the reference launches ~326
 * kernels per token). mode 0: 5 L + 2 launches (q/k/v, attention, o_proj, gate_up, down
 * per layer). mode 1: the persistent ring layer -- per layer the attention launch plus
 * ONE launch for o_proj, RMSNorm + gate_up + SiLU*up, down (K split by CU) and the next
 * layer's RMSNorm + q/k/v, one workgroup per CU whose loader waves stream the weights
 * through an LDS ring ahead of the in-launch hand-offs (2 L + 3 launches). Mode 1 needs
 * fp16 weights, hidden 4096, head_dim 128, heads dividing the CU count and tp_world 1
 * (else LLMI_EUNSUPPORTED); it keeps a transposed copy of every W_down (rebuilt after a
 * weight load). The two modes differ only in the down projection's fp32 summation order.
 * Graphs are re-captured. */
int llmi_engine_set_decode_mode(llmi_engine* e, int mode);

/* ---- One-shot peer exchange for tensor parallel decode (config 4; replaces the RCCL
 * all-reduces of the token graph: the sum of the row-parallel partials of
 * modeling_llama.py's pretraining_tp, :251-266 / :443-446, and the argmax-key max).
 * Every rank owns an inbox in its HBM; each exchange is ONE kernel that writes this rank's
 * int64 partial into every peer's inbox over xGMI, raises per-slice flags, waits for every
 * rank's flags and sums the slots in rank order (exact: bitwise the RCCL result).
 *   1. llmi_engine_xchg_handle: allocate the inbox, return its 64-byte IPC handle;
 *   2. the launcher all-gathers the handles (any side channel; rank order);
 *   3. llmi_engine_xchg_open(e, handles[world * 64]): map every peer's inbox;
 *   4. llmi_engine_set_exchange(e, 1) (0 = RCCL again; graphs are re-captured).
 *      Mode 2 runs the same protocol from INSIDE the producing launches: the o_proj, down
 *      and lm_head kernels end with an arrival ticket; their last workgroups push the
 *      finished vector to every inbox, wait for the peers and reduce in rank order (no
 *      exchange launch, 2 L + 1 fewer launches and kernel boundaries per token); results
 *      are bitwise those of modes 0 and 1.
 * A peer that never arrives (2 s) sets error bit 8: llmi_engine_tokens fails, no hang. */
int llmi_engine_xchg_handle(llmi_engine* e, void* out64);
int llmi_engine_xchg_open(llmi_engine* e, const void* handles);

/* One-GPU pricing of ONE tensor-parallel rank (no reference counterpart): a tp_world > 1
 * engine without peers runs its shard's whole token loop with every peer inbox replaced by
 * its own -- the push writes this rank's slice into its own slot and zeros into the W - 1
 * others (the same bytes a real push writes), raises all W flags, and the reduce sums to
 * this rank's own partial. Tokens are NOT the TP model's (the other ranks' partials are
 * zero); the launch / exchange structure and its timing are. set_exchange 0 then runs no
 * exchange at all (the compute-only floor), 1 the one-shot exchange launches, 2 the
 * exchange fused into the producers. */
int llmi_engine_xchg_loopback(llmi_engine* e);

/* Engine tuning switches for same-process A/B (no reference counterpart); the captured
 * token graphs are rebuilt on the next decode. "kpar": 1 (default) lets a TP rank's q/k/v and
 * gate_up GEMVs split K over 2 or 4 waves of a workgroup when one row group per wave would
 * leave CUs idle or doubled (tp_world > 1 only), 0 keeps one wave per row group.
 * "qkv_attn": 1 (default) runs a layer's q/k/v GEMV and split-KV attention as one launch (q/k/v
 * handed over as tagged 8-byte granules; bitwise the two launches), 0 as two. "qa_o": 1 adds the
 * o_proj to that launch (fp16 MHA, single rank; default 0, measured slower). "qa_grid" (workgroups
 * of the fused launch's GEMV part, 0 = every resident slot), "qa_order" (1 head-major rows and
 * attention blocks, default), "qa_poll" (1 poll every granule from the start): A/B only. */
int llmi_engine_set_option(llmi_engine* e, const char* name, int value);
int llmi_engine_set_exchange(llmi_engine* e, int mode);
/* Diagnostics: kernels launched by llmi_engine_time_kernel (and graphs built
 * afterwards) write a per-workgroup timeline into dev_buf (8 x uint64 per
 * workgroup at 8 * linear block id: start, two kernel-defined marks, end, CU id;
 * 100 MHz clock). NULL switches it off. */
int llmi_engine_debug_stamps(llmi_engine* e, void* dev_buf);
/* Graph-replay timeline: like llmi_engine_debug_stamps, but every stamped launch of a
 * recorded token step (qkv, attention, o_proj, gate_up, down per layer, then lm_head)
 * writes its own region of slot_wgs workgroups x 64 B, in launch order, so one replay of
 * a captured token graph leaves the whole step's per-workgroup timeline. Captured graphs
 * are dropped (re-captured with the stamp pointers on the next graph decode); launches
 * past bytes / (slot_wgs * 64) regions are not stamped. slot_wgs must cover the largest
 * decode grid (the error names the bound). dev_buf NULL switches it off. */
int llmi_engine_debug_timeline(llmi_engine* e, void* dev_buf, size_t bytes, int slot_wgs);
/* Test hook: overwrite the device decode state's next position only (the host's copy is
 * left alone), to check that a host/device position mismatch is reported (error bit 4). */
int llmi_engine_debug_set_next_pos(llmi_engine* e, int next_pos);

/* ---- In-process tensor-parallel group (no reference counterpart: the
 * reference has no TP). W rank engines with tp_rank 0..W-1 on ONE device and
 * one stream, stepped phase by phase with an in-place reduction kernel where
 * the RCCL path all-reduces. RCCL refuses two ranks on one device, so this is
 * the single-GPU parity harness for the sharded path (per-rank weight shards,
 * rank-0 residual, vocab-parallel argmax keys). cfg->tp_rank/tp_world are
 * ignored; the group sets them. Same status codes as the engine. */
typedef struct llmi_group llmi_group;
int llmi_group_create(const llmi_config* cfg, int world, int device, llmi_group** out);
int llmi_group_destroy(llmi_group* g);
int llmi_group_load_synthetic(llmi_group* g, uint64_t seed);
int llmi_group_load_bin(llmi_group* g, const char* weight_path);
/* llmi_engine_load_bin_quantized on every rank (int8 groups) */
int llmi_group_load_bin_quantized(llmi_group* g, const char* weight_path);
int llmi_group_set_prompt(llmi_group* g, const int32_t* ids, int n);
int llmi_group_decode(llmi_group* g, int n_steps, int use_graph);
/* tokens as seen by one rank (every rank must agree) */
int llmi_group_tokens(llmi_group* g, int rank, int32_t* out, int n, int* n_valid);
/* last logits over the full vocab: the ranks' slices concatenated */
int llmi_group_logits(llmi_group* g, float* out, int n);
int llmi_group_hidden(llmi_group* g, int rank, float* out, int n);
/* mode 0: the in-place reduction kernel; 1: the one-shot peer exchange's kernels (every
 * rank's push, then every rank's wait + rank-order reduce; the ranks' inboxes are the
 * group's own device buffers) -- the single-GPU parity check of that protocol; 2: the
 * push fused into every rank's o_proj / down / lm_head launch (their tails), then every
 * rank's reduce kernel (one stream: an in-launch wait for a later rank cannot finish). */
int llmi_group_set_exchange(llmi_group* g, int mode);

/* ---- Batched decode (no reference counterpart: the reference decodes one sequence). Up to
 * 8 sequence slots share ONE copy of the weights and one stream. A step advances every
 * active slot by one token: the q/k/v, gate_up, down and lm_head projections of all active
 * slots run as one multi-row GEMV each (every weight streamed once per step instead of once
 * per sequence); the attention + o_proj pair runs per slot at that slot's own position. A
 * slot decoded in a batch gives bitwise the tokens and logits it gives alone in an engine
 * with the same configuration, weights and sampling. Slots may hold prompts of different
 * lengths and sit at different positions; prompts are consumed by decode steps (no batched
 * prefill). A slot without a prompt is idle and costs nothing. Admission and eviction are the
 * caller's: llmi_batch_set_prompt (re)starts one slot, llmi_batch_reset makes it idle.
 * cfg->tp_world must be 1 (else LLMI_EUNSUPPORTED); n_seq in 1..8. */
typedef struct llmi_batch llmi_batch;
int llmi_batch_create(const llmi_config* cfg, int n_seq, int device, llmi_batch** out);
int llmi_batch_destroy(llmi_batch* b);
int llmi_batch_load_synthetic(llmi_batch* b, uint64_t seed);
int llmi_batch_load_bin(llmi_batch* b, const char* weight_path);
int llmi_batch_load_bin_quantized(llmi_batch* b, const char* weight_path);
int llmi_batch_set_prompt(llmi_batch* b, int seq, const int32_t* ids, int n);
int llmi_batch_reset(llmi_batch* b, int seq);
/* llmi_engine_edit of slot seq's sequence, on the batch's stream: the slot goes on bitwise as
 * the edited engine would alone, the other slots as if nothing happened. LLMI_EINVAL for a seq
 * out of range, an idle slot, and llmi_engine_edit's own. */
int llmi_batch_edit(llmi_batch* b, int seq, int keep, const int32_t* ids, int n);
/* Fork a slot (no reference counterpart): copy slot src's sequence -- cache rows, ids and decode
 * state -- into the n_dst (1..7) slots dst[], on the device and in stream order, so that n
 * continuations of one prompt cost one prompt pass. With P the source's next position
 * (keep = -1 means P), two forms:
 *   Cut (n >= 1, 0 <= keep <= P, keep + n <= max_seq): every destination becomes what the source
 * would be after llmi_batch_edit(b, src, keep, ids, n) -- rows [0, keep) of every layer's K and V
 * (and their KV8 scales) and ids [0, keep) are the source's bytes, positions keep .. keep + n - 1
 * take ids as a prompt would, the next position is keep and the prompt length keep + n, the
 * pending token is forgotten. It goes on bitwise as the edited source would. keep == 0 copies no
 * row: llmi_batch_set_prompt(ids) without its synchronise.
 *   Continue (n == 0, keep == P): every destination is the source as it stands, the pending token
 * included: also copied are the prompt and its length, the argmax partials, the raw logits row,
 * and the processed row where source and destination both have logit rules on. The next step of
 * a destination picks the token the source's next step picks; with a sampler, later tokens
 * follow the destination's own seed.
 *   Both: the source is only read and goes on as if nothing happened. A destination keeps its
 * own sampler, seed, logit rules, allowed set and logprob setting; whatever sequence it held is
 * gone, an idle one becomes active. Its device error word becomes the source's (a fork of a
 * faulted sequence is faulted); its forward counter is left alone. Logprob records are copied
 * where source and destination both have logprobs on with the same n_top -- records [0, keep) in
 * the cut form (record keep stays not computed, as after llmi_engine_edit), [0, P] in the
 * continue form -- and every other record of the destination becomes "not computed"; with any
 * other combination of settings all of them do. The destination's scored-prefill slab is
 * forgotten. The captured step graphs stay valid: no buffer moves.
 *   Two stream-ordered launches (kv_copy_rows_kernel, none for keep == 0; seq_fork_kernel). For
 * n <= 8 the ids travel in the launch arguments and the call neither copies nor synchronises; a
 * longer list is copied first and the call synchronises (as llmi_engine_edit).
 *   LLMI_EINVAL, with nothing changed: src out of range or idle; n_dst outside 1..7; a
 * destination out of range, equal to src or listed twice; keep or n outside the ranges above; an
 * id outside [0, vocab); n == 0 with keep != P (a cut needs a forced id: the pending token is
 * forgotten). */
int llmi_batch_fork(llmi_batch* b, int src, const int* dst, int n_dst, int keep, const int32_t* ids, int n);
/* llmi_engine_set_sampling_params for one slot: step = seed + the sampled token's position,
 * row 0, as in the engine. */
int llmi_batch_set_sampling_params(llmi_batch* b, int seq, const llmi_sampling_params* p);
/* llmi_engine_set_logit_rules / _set_allowed / _clear_logit_rules / _processed_logits for one
 * slot: the rules, the allowed set and the processed row are the slot's own (one launch per
 * active slot with rules on, before that slot's sampler), bitwise those of an engine running
 * the sequence alone. Replacing the contents of a slot's allowed set keeps the batch's
 * captured steps; every other change drops them. LLMI_EINVAL for a seq out of range. */
int llmi_batch_set_logit_rules(llmi_batch* b, int seq, const int32_t* bias_ids, const float* bias_values, int n_bias,
                               float presence_penalty, float frequency_penalty, int count_prompt);
int llmi_batch_set_allowed(llmi_batch* b, int seq, const int32_t* ids, int n);
int llmi_batch_clear_logit_rules(llmi_batch* b, int seq);
int llmi_batch_processed_logits(llmi_batch* b, int seq, float* out, int n);
/* llmi_engine_set_logprobs / llmi_engine_logprobs for one slot: the setting and the records are
 * the slot's own (one launch per active slot with logprobs on, after that slot's sampler), and
 * bitwise those of an engine running the sequence alone. llmi_batch_set_prompt clears only
 * that slot's records. */
int llmi_batch_set_logprobs(llmi_batch* b, int seq, int n_top);
int llmi_batch_logprobs(llmi_batch* b, int seq, float* tok_lp, int32_t* top_ids, float* top_lp, int n, int* n_valid,
                        int* n_top);
/* Every active slot advances n_steps tokens. LLMI_EINVAL if no slot is active or any active
 * slot would pass max_seq. use_graph: the step is captured per (active slots, their attention
 * split counts and logprob settings) in a bounded cache and replayed; replay is bitwise the eager step. */
int llmi_batch_decode(llmi_batch* b, int n_steps, int use_graph);
/* llmi_engine_prefill (scored != 0: llmi_engine_prefill_scored) of slot seq's next n_tokens
 * prompt rows, on the batch's stream. The other slots are untouched; the slot ends where
 * n_tokens decode steps would have left it, bitwise as an engine that prefilled alone, and
 * the next llmi_batch_decode steps it with the others. The prefill scratch, the e4m3 weight
 * copies of exact = 2 and the logits slab exist once per batch (slot 0 owns them, one stream
 * serialises their use); a llmi_batch_load_* drops the e4m3 copies. LLMI_EINVAL for a seq out
 * of range, an idle slot or rows past the slot's prompt. */
int llmi_batch_prefill(llmi_batch* b, int seq, int n_tokens, int exact, int scored);
int llmi_batch_tokens(llmi_batch* b, int seq, int32_t* out, int n, int* n_valid);
int llmi_batch_logits(llmi_batch* b, int seq, float* out, int n);
int llmi_batch_sync(llmi_batch* b);
/* Bytes one step over the currently active slots streams: the weights once, W_o (still read
 * per slot) once per active slot; and the KV bytes per cached position of one slot. */
int llmi_batch_bytes(llmi_batch* b, uint64_t* weight_bytes_per_step, uint64_t* kv_bytes_per_pos);

#ifdef __cplusplus
}
#endif
#endif /* LLMI_H_ */
