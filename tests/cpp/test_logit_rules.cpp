// LlamaModel::setLogitRules / setAllowedTokens / clearLogitRules + Response through the C++ model
// API: prints the generated ids, which tests/test_cpp_logit_rules.py compares with the Python
// engine's for the same settings. Without arguments it only has to compile and link (no device
// work); the Llama<T> methods are instantiated so that both classes are checked.
//   test_logit_rules weight_seed n_new bias_id bias_value banned_id presence frequency allowed_id n_prompt id...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "llmi/model.h"

static void print_ids(const char* key, const std::vector<int>& v) {
    std::printf("{\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]}\n");
}

// never called: the three methods of Llama<T> must compile for both instantiations
template <typename T>
void instantiate(Llama<T>& m) {
    m.setLogitRules({{1, 2.f}, {2, -INFINITY}}, 0.5f, 0.25f, true);
    m.setLogitRules({});
    m.setAllowedTokens({1, 2, 3});
    m.clearLogitRules();
}
template void instantiate<float>(Llama<float>&);
template void instantiate<half_t>(Llama<half_t>&);

int main(int argc, char** argv) {
    if (argc < 11) return 0;
    try {
        const uint64_t weight_seed = std::strtoull(argv[1], nullptr, 10);
        const int n_new = std::atoi(argv[2]);
        const int bias_id = std::atoi(argv[3]);
        const float bias_value = (float)std::atof(argv[4]);
        const int banned = std::atoi(argv[5]);
        const float presence = (float)std::atof(argv[6]), frequency = (float)std::atof(argv[7]);
        const int allowed_id = std::atoi(argv[8]);
        const int n_prompt = std::atoi(argv[9]);
        std::vector<int> prompt;
        for (int i = 10; i < argc && (int)prompt.size() < n_prompt; ++i) prompt.push_back(std::atoi(argv[i]));
        llm::LlamaModel m("tiny", LLMI_F16, LLMI_F32);
        m.loadWeightsFromDummy(weight_seed);
        m.setLogitRules({{bias_id, bias_value}, {banned, -INFINITY}}, presence, frequency, false);
        print_ids("rules", m.Response(prompt, n_new, nullptr, /*eos*/ -1));
        // the mask on top of the rules: one allowed id
        m.setAllowedTokens({allowed_id});
        print_ids("masked", m.Response(prompt, n_new, nullptr, -1));
        // an empty list removes the mask: the rules alone again
        m.setAllowedTokens({});
        print_ids("unmasked", m.Response(prompt, n_new, nullptr, -1));
        m.clearLogitRules();
        print_ids("greedy", m.Response(prompt, n_new, nullptr, -1));
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 2;
    }
    return 0;
}
