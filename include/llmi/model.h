// Model-level API.
//  * BaseModel / Llama<T> / llm::CreateModelWithName / CreateDummyLLMModel /
//    CreateRealLLMModel: the reference's string-in, string-out interface
//    (src/models/basemodel.h:14-42, src/models/llama/llama.h, llama.cpp:149-162
//    MakeInput/MakeHistory, :362-457 Response, src/utils/model_utils.h:17-82), so
//    user_entry.cpp compiles against this header with only its includes changed
//    (examples/user_entry.cpp). Response tokenizes the context (tokenizer.h), runs
//    the prompt as ONE batched prefill (firstTokenGen, llama.cpp:273-316) and then
//    the graph-replayed decode loop (continueTokenGen, :318-349) of the engine.
//  * LlamaModel: the same loop with token ids in and out.
#pragma once
#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "layers.h"
#include "tensor.h"
#include "tokenizer.h"

namespace llm {

// basemodel.h CallBack: index 0 = first generated token, -1 = end of the answer
using TokenCallBack = std::function<void(int index, int token)>;

// Log-probabilities of generated tokens (llmi_engine_set_logprobs): token[i] is the logprob of
// the i-th generated token under the raw logits it was chosen from; top_ids / top_logprobs
// [i * n_top + j] the j-th most likely id at that step and its logprob.
struct TokenLogprobs {
    int n_top = 0;
    std::vector<float> token;
    std::vector<int> top_ids;
    std::vector<float> top_logprobs;
};

// records [first, first + count) of the engine (the generated tokens of a Response)
// sparse (id, value) bias pairs -> llmi_engine_set_logit_rules' flat arrays
inline void SetLogitRules(llmi_engine* eng, const std::vector<std::pair<int, float>>& bias, float presence,
                          float frequency, bool count_prompt) {
    std::vector<int32_t> ids;
    std::vector<float> vals;
    for (const auto& b : bias) {
        ids.push_back(b.first);
        vals.push_back(b.second);
    }
    LLMI_CALL(llmi_engine_set_logit_rules(eng, ids.empty() ? nullptr : ids.data(), vals.empty() ? nullptr : vals.data(),
                                          (int)ids.size(), presence, frequency, count_prompt ? 1 : 0));
}
// an empty list removes the mask
inline void SetAllowedTokens(llmi_engine* eng, const std::vector<int>& ids) {
    const std::vector<int32_t> v(ids.begin(), ids.end());
    LLMI_CALL(llmi_engine_set_allowed(eng, v.empty() ? nullptr : v.data(), (int)v.size()));
}

inline TokenLogprobs ReadLogprobs(llmi_engine* eng, int first, int count) {
    TokenLogprobs r;
    int valid = 0;
    LLMI_CALL(llmi_engine_logprobs(eng, nullptr, nullptr, nullptr, 0, &valid, &r.n_top));
    const int n = std::min(valid, first + count);
    if (n <= first) return r;
    std::vector<float> lp(n), tlp((size_t)n * r.n_top);
    std::vector<int> ids((size_t)n * r.n_top);
    LLMI_CALL(llmi_engine_logprobs(eng, lp.data(), ids.data(), tlp.data(), n, &valid, &r.n_top));
    r.token.assign(lp.begin() + first, lp.end());
    r.top_ids.assign(ids.begin() + (size_t)first * r.n_top, ids.end());
    r.top_logprobs.assign(tlp.begin() + (size_t)first * r.n_top, tlp.end());
    return r;
}

class LlamaModel {
public:
    // preset: "llama2-7b", "llama2-13b", "tiny"; weight_dtype LLMI_F16 / LLMI_F32 / LLMI_I8 / LLMI_I4
    LlamaModel(const std::string& preset, int weight_dtype = LLMI_F16, int kv_dtype = LLMI_F16, int max_seq = 0,
               int device = 0) {
        LLMI_CALL(llmi_config_preset(preset.c_str(), &cfg));
        cfg.weight_dtype = weight_dtype;
        cfg.kv_dtype = kv_dtype;
        if (max_seq > 0) cfg.max_seq = max_seq;
        LLMI_CALL(llmi_engine_create(&cfg, device, nullptr, &eng));
    }
    ~LlamaModel() { llmi_engine_destroy(eng); }
    LlamaModel(const LlamaModel&) = delete;
    LlamaModel& operator=(const LlamaModel&) = delete;

    void loadWeightsFromDummy(uint64_t seed = 0) { LLMI_CALL(llmi_engine_load_synthetic(eng, seed)); }
    // Llama<T>::loadWeights(weight_path) (llama_weights.cc:41-53): weight_path + "<name>.bin", raw fp32
    void loadWeights(const std::string& weight_path) { LLMI_CALL(llmi_engine_load_bin(eng, weight_path.c_str())); }
    // the same files into an LLMI_I8 model: the linear weights are quantised to W8A16 on the device
    // (an LLMI_I4 model: q/k/v, gate_up and down to 4-bit groups of 128 columns, o_proj to W8A16)
    void loadWeightsQuantized(const std::string& weight_path) {
        LLMI_CALL(llmi_engine_load_bin_quantized(eng, weight_path.c_str()));
    }
    // Llama<T>::Sampling's top-k (llama.cpp:245-262) in the decode step; k = 0 (default) is greedy
    void setSampling(int k, uint64_t seed = 0) { LLMI_CALL(llmi_engine_set_sampling(eng, k, seed)); }
    // temperature / top-k / top-p / repetition-penalty sampling (llmi_engine_set_sampling_params; no
    // reference counterpart): replaces setSampling's sampler, and setSampling replaces this one
    void setSamplingParams(int top_k = 0, float top_p = 1.f, float temperature = 1.f, float repetition_penalty = 1.f,
                           uint64_t seed = 0) {
        const llmi_sampling_params p{top_k, top_p, temperature, repetition_penalty, seed};
        LLMI_CALL(llmi_engine_set_sampling_params(eng, &p));
    }
    // per-token log-probabilities of what Response generates (llmi_engine_set_logprobs): -1 off
    // (default), 0 the generated token's, 1..8 also that many alternatives; lastLogprobs reads them
    void setLogprobs(int n_top) { LLMI_CALL(llmi_engine_set_logprobs(eng, n_top)); }
    TokenLogprobs lastLogprobs() { return ReadLogprobs(eng, last_prompt, last_generated); }
    // logit rules in the token step (llmi_engine_set_logit_rules; no reference counterpart): a bias
    // per id (-INFINITY bans it), presence / frequency penalties over the generated ids (count_prompt:
    // the prompt's too), applied before the sampler or the greedy argmax reads the row
    void setLogitRules(const std::vector<std::pair<int, float>>& bias, float presence = 0, float frequency = 0,
                       bool count_prompt = false) {
        SetLogitRules(eng, bias, presence, frequency, count_prompt);
    }
    // only these ids may be generated (llmi_engine_set_allowed); an empty list removes the mask
    void setAllowedTokens(const std::vector<int>& ids) { SetAllowedTokens(eng, ids); }
    void clearLogitRules() { LLMI_CALL(llmi_engine_clear_logit_rules(eng)); }

    // Greedy generation (the reference's K = 1 top-k + sampling). tokens_per_sync
    // forwards run back to back (graph replays) between host reads, so the host
    // round trip the reference paid per token (llama.cpp:266,443) is amortised.
    std::vector<int> Response(const std::vector<int>& prompt, int output_token_limit, const TokenCallBack& cb = nullptr,
                              int eos_token_id = 2, int tokens_per_sync = 16) {
        LLM_CHECK_WITH_INFO(!prompt.empty(), "empty prompt");
        LLMI_CALL(llmi_engine_set_prompt(eng, prompt.data(), (int)prompt.size()));
        std::vector<int> out;
        std::vector<int> all(cfg.max_seq + 1);
        last_prompt = (int)prompt.size();
        last_generated = 0;
        int done = 0, emitted = 0;
        const int total = std::min<int>((int)prompt.size() - 1 + output_token_limit, cfg.max_seq);
        while (done < total) {
            const int n = std::min(tokens_per_sync, total - done);
            LLMI_CALL(llmi_engine_decode(eng, n, 1));
            done += n;
            int valid = 0;
            LLMI_CALL(llmi_engine_tokens(eng, all.data(), (int)all.size(), &valid));
            for (int p = (int)prompt.size() + emitted; p < valid && emitted < output_token_limit; ++p, ++emitted) {
                out.push_back(all[p]);
                last_generated = emitted + 1;
                if (cb) cb(emitted, all[p]);
                if (all[p] == eos_token_id) {
                    if (cb) cb(-1, -1);
                    return out;
                }
            }
        }
        if (cb) cb(-1, -1);
        return out;
    }
    std::vector<float> lastLogits() {
        std::vector<float> l(cfg.vocab);
        LLMI_CALL(llmi_engine_logits(eng, l.data(), cfg.vocab));
        return l;
    }
    const llmi_config& config() const { return cfg; }

private:
    llmi_config cfg{};
    llmi_engine* eng = nullptr;
    int last_prompt = 0, last_generated = 0;  // the last Response's prompt length and generated count
};

// token-id variants of model_utils.h:63-82 (preset name instead of the template type)
inline std::unique_ptr<LlamaModel> CreateRealLLMModel(const std::string& weight_path,
                                                      const std::string& preset = "llama2-7b",
                                                      int weight_dtype = LLMI_F16, bool quantize = false) {
    auto m = std::make_unique<LlamaModel>(preset, weight_dtype);
    if (quantize)  // weight_dtype LLMI_I8 / LLMI_I4: W8A16 / W4A16 from the fp32 files
        m->loadWeightsQuantized(weight_path);
    else
        m->loadWeights(weight_path);
    return m;
}

inline std::unique_ptr<LlamaModel> CreateDummyLLMModel(const std::string& preset = "llama2-7b",
                                                       int weight_dtype = LLMI_F16, uint64_t seed = 0) {
    auto m = std::make_unique<LlamaModel>(preset, weight_dtype);
    m->loadWeightsFromDummy(seed);
    return m;
}

}  // namespace llm

// ------------------------------------------------------------------ BaseModel
// basemodel.h:10 -- index 0 = first generated piece, > 0 the next ones, -1 = end
// (content = the whole answer)
using CallBack = std::function<void(int index, const char* GenerateContent)>;

// basemodel.h:14-42. The stream / blas handle / device properties are carried for
// source compatibility; the engine owns its own HIP stream.
class BaseModel {
public:
    std::string model_name;
    void* stream;
    cublasWrapper* cublas_wrapper;
    BaseAllocator* allocator;
    void* cuda_device_prop;
    BaseModel(void* stream, cublasWrapper* cublas_wrapper, BaseAllocator* allocator, void* cuda_device_prop = nullptr)
        : stream(stream), cublas_wrapper(cublas_wrapper), allocator(allocator), cuda_device_prop(cuda_device_prop) {}
    virtual ~BaseModel() = default;
    virtual void loadTokenizer(std::string file) = 0;
    virtual void loadWeights(std::string file) = 0;
    virtual void loadWeightsFromDummy() = 0;
    virtual std::vector<std::string> MakeInput(const std::string& history, int round, const std::string& input) = 0;
    virtual std::string MakeHistory(const std::string& history, int round, const std::string& input,
                                    const std::string& output) = 0;
    virtual std::string Response(const std::vector<std::string>& input, CallBack PrintRes) = 0;
};

// llama.h: Llama<T> with T = float (the reference's working instantiation: fp32
// weights, fp32 KV cache) or half_t (fp16 weights and KV cache: the throughput
// engine). Same constructor arguments as llama.h:88-101.
template <typename T>
class Llama : public BaseModel {
    static_assert(std::is_same<T, float>::value || std::is_same<T, half_t>::value, "Llama<T>: T = float or half_t");

public:
    Llama(int head_num, int kv_head_num, int head_size, int inter_size, int num_layers, int vocab_size,
          const LLaMAAttentionStaticParams& attn_static_params, int max_seq_len, void* stream,
          cublasWrapper* cublas_wrapper, BaseAllocator* allocator, void* cuda_device_prop = nullptr, int device = 0)
        : BaseModel(stream, cublas_wrapper, allocator, cuda_device_prop) {
        model_name = "llama";
        cfg.hidden = head_num * head_size;
        cfg.heads = head_num;
        cfg.kv_heads = kv_head_num;
        cfg.head_dim = head_size;
        cfg.inter = inter_size;
        cfg.layers = num_layers;
        cfg.vocab = vocab_size;
        cfg.max_seq = max_seq_len;
        cfg.rms_eps = rmsnorm_eps;
        cfg.rope_base = attn_static_params.rotary_embedding_base;
        cfg.weight_dtype = std::is_same<T, float>::value ? LLMI_F32 : LLMI_F16;
        cfg.kv_dtype = cfg.weight_dtype;
        cfg.tp_rank = 0;
        cfg.tp_world = 1;
        LLMI_CALL(llmi_engine_create(&cfg, device, nullptr, &eng));
    }
    ~Llama() override { llmi_engine_destroy(eng); }
    Llama(const Llama&) = delete;
    Llama& operator=(const Llama&) = delete;

    void loadTokenizer(std::string file) override { tokenizer.Initialize(file); }
    // llama_weights.cc:41-53: weight_path + "<name>.bin", raw fp32 per tensor
    void loadWeights(std::string file) override { LLMI_CALL(llmi_engine_load_bin(eng, file.c_str())); }
    // layer_weights.cc dummy path -> llmi-prng-v1 synthetic weights
    void loadWeightsFromDummy() override { LLMI_CALL(llmi_engine_load_synthetic(eng, dummy_seed)); }

    // llama.cpp:149-156: {history + input (round > 0), history, input}
    std::vector<std::string> MakeInput(const std::string& history, int round, const std::string& input) override {
        return {(round == 0 ? "" : history) + input, history, input};
    }
    // llama.cpp:159-162
    std::string MakeHistory(const std::string& history, int round, const std::string& input,
                            const std::string& output) override {
        return (round == 0 ? prompt : history) + input + output;
    }

    // llama.cpp:362-457. input[0] (history + query) is tokenized with BOS first (the
    // ids the reference hard-codes at llama.cpp:371,382 are exactly that), prefilled in
    // one batched pass, then decoded until EOS, output_token_limit or max_seq. Every
    // generated piece goes to PrintRes(index, piece); PrintRes(-1, answer) at the end.
    std::string Response(const std::vector<std::string>& input, CallBack PrintRes) override {
        LLM_CHECK_WITH_INFO(!input.empty(), "Response: empty input (use MakeInput)");
        std::vector<int> ids = {bos_token_id};
        const std::vector<int> body = tokenizer.Encode(input[0]);
        ids.insert(ids.end(), body.begin(), body.end());
        // a history longer than the context window keeps BOS and its most recent half
        // (the reference has no policy: its fixed buffers overflow)
        if ((int)ids.size() >= cfg.max_seq) {
            const int keep = cfg.max_seq / 2;
            ids.erase(ids.begin() + 1, ids.end() - (keep - 1));
        }
        LLMI_CALL(llmi_engine_set_prompt(eng, ids.data(), (int)ids.size()));
        last_prompt = (int)ids.size();
        last_generated = 0;
        if (score_prompt_)  // firstTokenGen, the prompt's records filled
            LLMI_CALL(llmi_engine_prefill_scored(eng, (int)ids.size(), 1));
        else
            LLMI_CALL(llmi_engine_prefill(eng, (int)ids.size(), 1));  // firstTokenGen
        std::string res;
        std::vector<int> all(cfg.max_seq + 1);
        const int limit = std::min(output_token_limit, cfg.max_seq - (int)ids.size() + 1);
        int produced = 0, valid = 0;
        bool done = false;
        while (!done) {
            LLMI_CALL(llmi_engine_tokens(eng, all.data(), (int)all.size(), &valid));
            for (int p = (int)ids.size() + produced; p < valid && !done; ++p) {
                const int tok = all[p];
                if (produced > 0 && tok == eos_token_id) {  // llama.cpp:420-422
                    done = true;
                    break;
                }
                const std::string piece = tokenizer.Decode({tok});
                res += piece;
                if (PrintRes) PrintRes(produced, piece.c_str());
                last_generated = produced + 1;
                if (++produced >= limit) done = true;
            }
            if (done) break;
            // continueTokenGen: graph replays, several tokens per host read
            const int n = std::min(tokens_per_sync, limit - produced);
            LLMI_CALL(llmi_engine_decode(eng, n, 1));
        }
        if (PrintRes) PrintRes(-1, res.c_str());
        return res;
    }

    // Response samples with temperature / top-k / top-p / repetition penalty instead of
    // greedy argmax (llmi_engine_set_sampling_params; the reference has no such control)
    void setSamplingParams(int top_k = 0, float top_p = 1.f, float temperature = 1.f, float repetition_penalty = 1.f,
                           uint64_t seed = 0) {
        const llmi_sampling_params p{top_k, top_p, temperature, repetition_penalty, seed};
        LLMI_CALL(llmi_engine_set_sampling_params(eng, &p));
    }

    // logit rules in the token step (llmi_engine_set_logit_rules / llmi_engine_set_allowed; the
    // reference has no such control): as LlamaModel's
    void setLogitRules(const std::vector<std::pair<int, float>>& bias, float presence = 0, float frequency = 0,
                       bool count_prompt = false) {
        llm::SetLogitRules(eng, bias, presence, frequency, count_prompt);
    }
    void setAllowedTokens(const std::vector<int>& ids) { llm::SetAllowedTokens(eng, ids); }
    void clearLogitRules() { LLMI_CALL(llmi_engine_clear_logit_rules(eng)); }

    // per-token log-probabilities of the pieces Response generates (llmi_engine_set_logprobs: -1
    // off, 0 the token's own, 1..8 also that many alternatives), read by lastLogprobs. The
    // prompt itself is prefilled in one batched pass; score_prompt: that pass is the scored
    // prefill (llmi_engine_prefill_scored), so the prompt's own records are filled too and
    // lastPromptLogprobs reads them ("echo" logprobs). What Response generates is the same.
    void setLogprobs(int n_top) { setLogprobs(n_top, false); }
    void setLogprobs(int n_top, bool score_prompt) {
        LLMI_CALL(llmi_engine_set_logprobs(eng, n_top));
        score_prompt_ = n_top >= 0 && score_prompt;
    }
    llm::TokenLogprobs lastLogprobs() { return llm::ReadLogprobs(eng, last_prompt, last_generated); }
    // records 1 .. prompt length - 1: prompt token p under the forward at p - 1 (score_prompt)
    llm::TokenLogprobs lastPromptLogprobs() { return llm::ReadLogprobs(eng, 1, last_prompt - 1); }

    // the generated ids of the last Response (for tests and callers that keep ids)
    std::vector<int> lastTokens() {
        std::vector<int> all(cfg.max_seq + 1);
        int valid = 0;
        LLMI_CALL(llmi_engine_tokens(eng, all.data(), (int)all.size(), &valid));
        all.resize(valid);
        return all;
    }
    const llmi_config& config() const { return cfg; }
    Tokenizer& getTokenizer() { return tokenizer; }

    int output_token_limit = 256;  // llama.h:29
    int bos_token_id = 1, eos_token_id = 2;
    int tokens_per_sync = 16;
    uint64_t dummy_seed = 0;
    std::string prompt = "";  // llama.h:42 built-in prompt for round 0 of MakeHistory

private:
    float rmsnorm_eps = 1e-5f;  // llama.h:22
    llmi_config cfg{};
    llmi_engine* eng = nullptr;
    int last_prompt = 0, last_generated = 0;
    bool score_prompt_ = false;
    Tokenizer tokenizer;
};

namespace llm {

// model_utils.h:17-61 -- the reference's dummy geometry: Llama-2-7B widths, 3 layers,
// max_seq_len 64 (its debugging configuration), rope base 10000.
template <typename T>
BaseModel* CreateModelWithName(const std::string& model_name) {
    LLM_CHECK_WITH_INFO(model_name == "llama", "dont support other models except llama yet!");
    const int head_num = 32, kv_head_num = 32, head_size = 128, inter_size = 11008, num_layers = 3;
    const int max_seq_len = 64, vocab_size = 32000;
    LLaMAAttentionStaticParams attn_static_params;
    attn_static_params.rotary_embedding_dim = 128;
    attn_static_params.rotary_embedding_base = 10000;
    attn_static_params.max_position_embeddings = 4096;
    attn_static_params.use_dynamic_ntk = false;
    static HipAllocator allocator;
    return new Llama<T>(head_num, kv_head_num, head_size, inter_size, num_layers, vocab_size, attn_static_params,
                        max_seq_len, nullptr, nullptr, &allocator);
}

// model_utils.h:63-70
template <typename T>
std::unique_ptr<BaseModel> CreateDummyLLMModel(std::string tokenizer_file) {
    BaseModel* model = CreateModelWithName<T>("llama");
    std::unique_ptr<BaseModel> owned(model);
    model->loadTokenizer(tokenizer_file);
    model->loadWeightsFromDummy();
    return owned;
}

// model_utils.h:73-82
template <typename T>
std::unique_ptr<BaseModel> CreateRealLLMModel(std::string model_dir, std::string tokenizer_file) {
    BaseModel* model = CreateModelWithName<T>("llama");
    std::unique_ptr<BaseModel> owned(model);
    model->loadTokenizer(tokenizer_file);
    model->loadWeights(model_dir);
    return owned;
}

}  // namespace llm
