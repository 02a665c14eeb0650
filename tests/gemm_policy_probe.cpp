// Stand-alone probe of the pure GEMM host policy (yat_amd/csrc/gemm_policy.hpp): reads one query per line from stdin,
//   a_t b_t M N K K2 class wide_ok a2_group workspace_MiB word
// and prints one pick per line: -1 = refused, else tile * 10000 + ksplit * 100 + group.
// Built by tests/test_gemm_policy_cpu.py with a plain host compiler -- no HIP, no GPU.
#include <cstdio>

#include "../yat_amd/csrc/gemm_policy.hpp"

int main() {
    int a_t, b_t, M, N, K, K2, epi, wide, a2_group, ws_mib, word;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &a_t, &b_t, &M, &N, &K, &K2, &epi, &wide, &a2_group, &ws_mib, &word) == 11) {
        GemmQuery q{};
        q.a_t = a_t != 0; q.b_t = b_t != 0;
        q.M = M; q.N = N; q.K = K; q.K2 = K2;
        q.epi = (GemmEpi)epi;
        q.wide_ok = wide != 0;
        q.a2_group = a2_group;
        q.has_workspace = ws_mib > 0;
        q.workspace_bytes = (uint64_t)ws_mib << 20;
        GemmWord w{};
        GemmPlan plan{};
        int rc = decode_gemm_word(word, w);
        if (rc == YAT_OK) rc = gemm_plan(q, w, plan);
        printf("%d\n", rc == YAT_OK ? plan.tile * 10000 + plan.ksplit * 100 + plan.group : -1);
    }
    return 0;
}
