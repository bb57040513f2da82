// Llama<T>::setLogprobs(n_top, score_prompt) through the C++ model API: Response prefills the
// prompt with the scored form, lastPromptLogprobs reads the prompt's own records. Prints the
// prompt ids, the generated ids and the records (raw bits), which
// tests/test_cpp_prompt_logprobs.py compares with the Python engine's scored prefill. Without
// arguments it only has to compile and link (no device work).
//   test_prompt_logprobs tokenizer_file n_new n_top
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "llmi/model.h"

static unsigned bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return u;
}
static void print_ints(const char* key, const std::vector<int>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]");
}
static void print_bits(const char* key, const std::vector<float>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%u", i ? ", " : "", bits(v[i]));
    std::printf("]");
}
static void print_records(const char* prefix, const llm::TokenLogprobs& lp) {
    const std::string p(prefix);
    print_bits((p + "logprob_bits").c_str(), lp.token);
    std::printf(", ");
    print_ints((p + "top_ids").c_str(), lp.top_ids);
    std::printf(", ");
    print_bits((p + "top_logprob_bits").c_str(), lp.top_logprobs);
}

int main(int argc, char** argv) {
    if (argc < 4) {
        // both overloads and the reader exist in the model class
        void (Llama<float>::*set1)(int) = &Llama<float>::setLogprobs;
        void (Llama<half_t>::*set2)(int, bool) = &Llama<half_t>::setLogprobs;
        llm::TokenLogprobs (Llama<half_t>::*get)() = &Llama<half_t>::lastPromptLogprobs;
        return (set1 && set2 && get) ? 0 : 1;
    }
    try {
        const std::string query = "Hey, are you conscious? Can you talk to me?";
        static HipAllocator alloc;
        LLaMAAttentionStaticParams sp;
        // the tiny preset's geometry (4 heads x 128, inter 1024, 2 layers, 64 positions)
        Llama<half_t> model(4, 4, 128, 1024, 2, 32000, sp, 64, nullptr, nullptr, &alloc);
        model.loadTokenizer(argv[1]);
        model.loadWeightsFromDummy();
        model.output_token_limit = std::atoi(argv[2]);
        model.eos_token_id = -1;  // synthetic weights: generate the full budget
        const int n_top = std::atoi(argv[3]);
        model.setLogprobs(n_top, true);
        (void)model.Response(model.MakeInput("", 0, query), nullptr);
        const std::vector<int> all = model.lastTokens();
        const int n_prompt = 1 + (int)model.getTokenizer().Encode(query).size();
        const llm::TokenLogprobs plp = model.lastPromptLogprobs(), glp = model.lastLogprobs();
        std::printf("{\"n_top\": %d, ", plp.n_top);
        print_ints("prompt", std::vector<int>(all.begin(), all.begin() + n_prompt));
        std::printf(", ");
        print_ints("tokens", std::vector<int>(all.begin() + n_prompt, all.end()));
        std::printf(", ");
        print_records("prompt_", plp);
        std::printf(", ");
        print_records("", glp);
        std::printf("}\n");
        // without score_prompt the prompt's records stay "not computed" and the answer is the same
        model.setLogprobs(n_top);
        (void)model.Response(model.MakeInput("", 0, query), nullptr);
        const llm::TokenLogprobs off = model.lastPromptLogprobs();
        bool all_nan = !off.token.empty();
        for (float v : off.token) all_nan = all_nan && v != v;
        std::printf("{\"plain_prompt_not_computed\": %s, \"plain_same_tokens\": %s}\n", all_nan ? "true" : "false",
                    model.lastTokens() == all ? "true" : "false");
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 2;
    }
    return 0;
}
