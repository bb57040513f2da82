// Editing a sequence in place (engine.h; include/llmi.h has the contract): keep the first `keep`
// consumed positions, forget the pending token and everything after them, and force the ids of
// the positions that follow -- a rewind, an appended turn, or a draft engine taking the token its
// target chose. One stream-ordered launch on the engine's own buffers (DecodeState, prompt, the
// logprob records); the KV cache, the token history and the captured step graphs are left as
// they are: rows and ids at or after `keep` are stale and are rewritten by the step that
// reaches them before anything reads them (the argument for a verify step's rejected rows).
#include "engine.h"

namespace llmi {
namespace {

constexpr int kEditT = 256;
constexpr int kEditByValue = 8;  // ids that travel in the launch arguments

struct EditIds {
    int32_t v[kEditByValue];
};

// Workgroup 0, thread 0: the decode state (error and epoch stay: the fused q/k/v launch's
// granule tags must never repeat) and the n_val by-value ids into prompt[keep ..] (a longer
// list was copied there before the launch). All workgroups: the logprob records >= keep back
// to "not computed" (every byte 0xFF: NaN / id -1); lp_w0 = keep * the record stride of the
// two top arrays, lp_w1 their length in words.
__global__ __launch_bounds__(kEditT) void seq_edit_kernel(DecodeState* st, int32_t* prompt, int keep, int n,
                                                          EditIds ids, int n_val, unsigned* lp_tok, unsigned* lp_ids,
                                                          unsigned* lp_tlp, int records, size_t lp_w0, size_t lp_w1) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->next_pos = keep;
        st->cur_pos = keep > 0 ? keep - 1 : 0;
        st->prompt_len = keep + n;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < n_val) prompt[keep + threadIdx.x] = ids.v[threadIdx.x];
    if (!lp_tok) return;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t q = (size_t)keep + t; q < (size_t)records; q += step) lp_tok[q] = 0xFFFFFFFFu;
    for (size_t i = lp_w0 + t; i < lp_w1; i += step) {
        lp_ids[i] = 0xFFFFFFFFu;
        lp_tlp[i] = 0xFFFFFFFFu;
    }
}

}  // namespace

int Engine::edit(int keep, const int32_t* ids, int n) {
    if (decode_mode == 1) {
        set_last_error("[llmi][ERROR] edit: the ring decode mode keeps a sequence it cannot rewind (set_decode_mode 0)");
        return LLMI_EUNSUPPORTED;
    }
    LLMI_REQUIRE(prompt_len > 0, "edit: set_prompt first");
    LLMI_REQUIRE(keep >= 0 && keep <= host_next_pos, "edit: keep must be in [0, next position]");
    LLMI_REQUIRE(n >= 0 && n <= c.max_seq - keep, "edit: need n >= 0 and keep + n <= max_seq");
    LLMI_REQUIRE(n == 0 || ids != nullptr, "edit: null ids");
    for (int i = 0; i < n; ++i) LLMI_REQUIRE(ids[i] >= 0 && ids[i] < c.vocab, "edit: token id out of range");
    if (keep == host_next_pos && n == 0) return LLMI_OK;
    LLMI_REQUIRE(n >= 1, "edit: a rewind needs at least one forced id (the pending token is forgotten)");
    EditIds v{};
    const int n_val = n <= kEditByValue ? n : 0;
    for (int i = 0; i < n_val; ++i) v.v[i] = ids[i];
    if (n_val == 0) LLMI_HIP(hipMemcpyAsync(prompt + keep, ids, (size_t)n * 4, hipMemcpyHostToDevice, stream));
    const int records = (int)lp_records();
    const size_t w0 = lp_buf ? (size_t)keep * (size_t)std::max(lp_stride, 0) : 0;
    const size_t w1 = lp_buf ? lp_records() * kLpMaxTop : 0;
    const size_t work = lp_buf ? std::max((size_t)(records - keep), w1 - w0) : 1;
    const int grid = (int)std::min<size_t>(64, (work + kEditT - 1) / kEditT);
    hipLaunchKernelGGL(seq_edit_kernel, dim3(std::max(grid, 1)), dim3(kEditT), 0, stream, st, prompt, keep, n, v, n_val,
                       reinterpret_cast<unsigned*>(lp_buf ? lp_tok() : nullptr),
                       reinterpret_cast<unsigned*>(lp_buf ? lp_ids() : nullptr),
                       reinterpret_cast<unsigned*>(lp_buf ? lp_tlp() : nullptr), records, w0, w1);
    LLMI_HIP(hipGetLastError());
    if (n_val == 0) LLMI_HIP(hipStreamSynchronize(stream));  // the caller's ids were read from pageable memory
    host_next_pos = keep;
    prompt_len = keep + n;
    sc_m = 0;  // the logits slab holds no row of this sequence
    return LLMI_OK;
}

}  // namespace llmi
