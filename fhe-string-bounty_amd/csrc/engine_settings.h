// engine_settings.h -- every setting of an engine: its default, its range and its environment name, here and nowhere else.
// Host only, standard headers only (tests/engine_settings_main.cpp compiles it with a plain C++17 compiler).
//
// Two ways in, which differ on purpose:
//   from_env()  read once by Engine::create.  The environment switches exist for diagnostics and A/B measurements (scripts/):
//               an unset variable leaves the default, a set one is read with atoi (text that is no number is 0), a value
//               below the accepted range is ignored and one above it is clamped.
//   set_*()     the product interface, one per fhe_engine_set_* (c_api.cpp).  A value out of range is refused: the setter
//               returns the error text and changes nothing; nullptr = accepted.
// fhe_engine_set_variant and fhe_engine_set_pipeline are engine operations (they pick kernels / synchronise first), not
// stored settings; the variant's selector at creation is read here because it has an environment name.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdlib>

namespace fhe {

struct EngineSettings {
    // ranges
    static constexpr int WIDE_FAIR_MAX = 20;
    static constexpr int OVERLAP_MIN = 2, OVERLAP_MAX = 4;         // OVERLAP_MAX is Pipeline::MAX_LANES (engine.h asserts it)
    static constexpr int CLUSTER_MODE_MIN = -1, CLUSTER_MODE_MAX = 2;
    static constexpr int CLUSTER_SPIN_MIN = 64;
    static constexpr int MULTIBIT_COMBINE_LIMIT = 1024;            // the workspace grows by 16 MB per LWE at N = 2048

    int variant_selector = 0;                  // FHESTR_LOG2_POINTS          blind-rotation variant at creation (fhe_engine_set_variant)
    uint32_t wide_fair_shift = 13;             // FHESTR_WIDE_FAIR            two-LWEs-per-CU kernel: log2 ticks (100 MHz) of the priority time slice, 0 = off
    uint32_t dense_per_cu = 2;                 // FHESTR_DENSE_PER_CU         N = 1024, k = 2: the four-workgroups-per-CU kernel beyond this many LWEs per CU (0 = never)
    bool cluster_fallback = true;              // FHESTR_CLUSTER_FALLBACK     a multi-CU launch that gave up is re-run on the one-workgroup kernel; 0: it is an error
    bool keep_busy = false;                    // FHESTR_KEEP_BUSY            small launches carry replicas on the idle CUs (fhe_engine_set_keep_busy)
    int overlap_width = OVERLAP_MIN;           // FHESTR_OVERLAP_STREAMS      lanes of throughput mode 2 (Pipeline::width)
    bool ks_mfma_enabled = true;               // FHESTR_KS_MFMA              0: byte-plane dot4 keyswitch kernel everywhere
    uint32_t ks_chunks_override = 0;           // FHESTR_KS_CHUNKS            K chunks of the matrix-core keyswitch (0 = automatic)
    int cluster_mode = -1;                     // FHESTR_CLUSTER              -1 automatic (by batch size), 0 never, 1 always, 2 always the 8-CU clusters (fhe_engine_set_cluster_mode)
    uint32_t cluster_max_batch = 0xFFFFFFFFu;  //                             automatic mode: batches up to this size take a multi-CU kernel (fhe_engine_set_cluster_mode)
    uint32_t cluster_spin_limit = 1u << 22;    // FHESTR_CLUSTER_SPIN_LIMIT   polls before a hand-over wait gives up
    uint32_t multibit_combine_max = 64;        // FHESTR_MULTIBIT_COMBINE_MAX multi-bit PBS: batches up to this size prepare their GGSWs on the whole GPU first
    size_t multibit_workspace_cap = 0;         // FHESTR_MULTIBIT_WS_CAP      bytes of prepared GGSWs (+ rotation workspace) the two-kernel multi-bit path keeps at once;
                                               //                             larger batches run in sub-batches (0 = from free memory; an int: up to 2 GB)
    uint32_t cluster_test_fault = 0;           // FHESTR_CLUSTER_TEST_FAULT   tests only, -DFHESTR_TEST_HOOKS builds only: epoch one workgroup stays silent at
    uint32_t xcd_auto_max = 16;                //                             automatic mode: batches up to this size take the whole-XCD kernel (two LWEs per XCD in flight)

    static EngineSettings from_env() {
        EngineSettings s;
        int v = 0;
        // is the variable set, to at least `least`?  Its value is then in v.
        auto read = [&v](const char* name, int least = 0) {
            const char* t = getenv(name);
            if (t) v = atoi(t);
            return t && v >= least;
        };
        if (read("FHESTR_LOG2_POINTS", INT_MIN)) s.variant_selector = v;
        if (read("FHESTR_WIDE_FAIR")) s.wide_fair_shift = (uint32_t)std::min(WIDE_FAIR_MAX, v);
        if (read("FHESTR_DENSE_PER_CU")) s.dense_per_cu = (uint32_t)v;
        if (read("FHESTR_CLUSTER_FALLBACK")) s.cluster_fallback = v != 0;
        if (read("FHESTR_KEEP_BUSY")) s.keep_busy = v != 0;
        if (read("FHESTR_OVERLAP_STREAMS")) s.overlap_width = std::min(OVERLAP_MAX, std::max(OVERLAP_MIN, v));
        if (read("FHESTR_KS_MFMA")) s.ks_mfma_enabled = v != 0;
        if (read("FHESTR_KS_CHUNKS")) s.ks_chunks_override = (uint32_t)v;
        if (read("FHESTR_CLUSTER", CLUSTER_MODE_MIN)) s.cluster_mode = std::min(CLUSTER_MODE_MAX, v);
        if (read("FHESTR_CLUSTER_SPIN_LIMIT")) s.cluster_spin_limit = (uint32_t)std::max(CLUSTER_SPIN_MIN, v);
        if (read("FHESTR_MULTIBIT_COMBINE_MAX")) s.multibit_combine_max = (uint32_t)std::min(MULTIBIT_COMBINE_LIMIT, v);
        if (read("FHESTR_MULTIBIT_WS_CAP", 1)) s.multibit_workspace_cap = (size_t)v;
#ifdef FHESTR_TEST_HOOKS      // fault injection exists only in the test build (make testhooks), never in the product library
        if (read("FHESTR_CLUSTER_TEST_FAULT")) s.cluster_test_fault = (uint32_t)v;
#endif
        return s;
    }

    const char* set_cluster_mode(int mode, uint32_t max_batch) {
        if (mode < CLUSTER_MODE_MIN || mode > CLUSTER_MODE_MAX)
            return "cluster mode: -1 (automatic), 0 (never), 1 (always) or 2 (always, the 8-CU clusters of round 3)";
        cluster_mode = mode;
        cluster_max_batch = max_batch;
        return nullptr;
    }
    const char* set_multibit_combine_max(uint32_t max_batch) {
        if (max_batch > (uint32_t)MULTIBIT_COMBINE_LIMIT) return "multibit_combine_max: at most 1024 (workspace grows by 16 MB per LWE at N = 2048)";
        multibit_combine_max = max_batch;
        return nullptr;
    }
    void set_keep_busy(int on) { keep_busy = on != 0; }      // any int
};

}  // namespace fhe
