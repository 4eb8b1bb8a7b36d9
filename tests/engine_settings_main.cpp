// engine_settings_main.cpp -- csrc/engine_settings.h on its own, for tests/test_engine_settings.py: the settings an engine
// would start with in this process's environment, then the API setters named on the command line, then every setting as a
// `name=value` line.  Arguments: cluster_mode=MODE,MAX_BATCH  combine_max=N  keep_busy=N; each prints `accepted NAME` or
// `refused NAME: <error text>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../fhe-string-bounty_amd/csrc/engine_settings.h"

int main(int argc, char** argv) {
    fhe::EngineSettings s = fhe::EngineSettings::from_env();
    for (int i = 1; i < argc; i++) {
        char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        *eq = 0;
        const char* name = argv[i];
        const char* why = nullptr;
        if (!strcmp(name, "cluster_mode")) {
            char* comma = nullptr;
            const long mode = strtol(eq + 1, &comma, 10);
            if (*comma != ',') { fprintf(stderr, "cluster_mode=MODE,MAX_BATCH\n"); return 2; }
            why = s.set_cluster_mode((int)mode, (uint32_t)strtoul(comma + 1, nullptr, 10));
        } else if (!strcmp(name, "combine_max")) {
            why = s.set_multibit_combine_max((uint32_t)strtoul(eq + 1, nullptr, 10));
        } else if (!strcmp(name, "keep_busy")) {
            s.set_keep_busy((int)strtol(eq + 1, nullptr, 10));
        } else {
            fprintf(stderr, "unknown setter %s\n", name);
            return 2;
        }
        if (why) printf("refused %s: %s\n", name, why);
        else printf("accepted %s\n", name);
    }
    printf("variant_selector=%d\n", s.variant_selector);
    printf("wide_fair_shift=%u\n", s.wide_fair_shift);
    printf("dense_per_cu=%u\n", s.dense_per_cu);
    printf("cluster_fallback=%d\n", (int)s.cluster_fallback);
    printf("keep_busy=%d\n", (int)s.keep_busy);
    printf("overlap_width=%d\n", s.overlap_width);
    printf("ks_mfma_enabled=%d\n", (int)s.ks_mfma_enabled);
    printf("ks_chunks_override=%u\n", s.ks_chunks_override);
    printf("cluster_mode=%d\n", s.cluster_mode);
    printf("cluster_max_batch=%u\n", s.cluster_max_batch);
    printf("cluster_spin_limit=%u\n", s.cluster_spin_limit);
    printf("multibit_combine_max=%u\n", s.multibit_combine_max);
    printf("multibit_workspace_cap=%zu\n", s.multibit_workspace_cap);
    printf("cluster_test_fault=%u\n", s.cluster_test_fault);
    printf("xcd_auto_max=%u\n", s.xcd_auto_max);
    return 0;
}
