// csrc/glwe_narrow.cpp under a host sanitizer (tests/test_glwe_narrow_host.py): narrow, widen and sample extraction over
// (N, k) x bits x held, every list allocated on the heap at exactly narrow_len words -- a read or write one word past it is
// a report -- and every output at exactly its size.  held covers 1, N - 1, N, N + 1, 2 N + 1 and, per width, the values
// whose last stream ends exactly on a u64 boundary and one bit short of one (odd widths only: an even width times any
// field count is even).  Prints one line per case: N k bits held, then the checksums sum of word_i (2 i + 1) mod 2^64 of
// the list, the widened GLWEs and the rows of every range, which the test compares with tests/exact_narrow.py.
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <set>
#include <vector>

#include "../fhe-string-bounty_amd/csrc/glwe_narrow.h"

static uint64_t splitmix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t checksum(const uint64_t* w, size_t n) {
    uint64_t s = 0;
    for (size_t i = 0; i < n; i++) s += w[i] * (2 * (uint64_t)i + 1);
    return s;
}

static int run(uint32_t N, uint32_t k, uint32_t bits, uint32_t held) {
    const size_t glwe_len = (size_t)(k + 1) * N, n_glwe = ((size_t)held + N - 1) / N, words = fhe::narrow_len(N, k, held, bits);
    if (!words) return 1;
    std::unique_ptr<uint64_t[]> glwes(new uint64_t[n_glwe * glwe_len]), narrow(new uint64_t[words]), wide(new uint64_t[n_glwe * glwe_len]);
    const uint64_t seed = ((uint64_t)N << 40) ^ ((uint64_t)k << 32) ^ ((uint64_t)bits << 24) ^ held;
    for (size_t i = 0; i < n_glwe * glwe_len; i++) glwes[i] = splitmix(seed + (i + 1) * 0x9E3779B97F4A7C15ull);
    for (size_t i = 0; i < words; i++) narrow[i] = ~0ull;                 // every word must be written, tail bits included
    if (fhe::glwe_narrow(N, k, glwes.get(), held, bits, narrow.get())) return 1;
    if (fhe::narrow_tail_check(N, k, narrow.get(), held, bits)) return 1;
    if (fhe::glwe_widen(N, k, narrow.get(), held, bits, wide.get())) return 1;
    printf("%u %u %u %u %016llx %016llx", N, k, bits, held, (unsigned long long)checksum(narrow.get(), words),
           (unsigned long long)checksum(wide.get(), n_glwe * glwe_len));
    // the ranges of tests/exact_extract.py, clipped to the blocks held
    const uint32_t ranges[5][2] = {{0, 1}, {0, N}, {N - 1, 2}, {3, N + 5}, {0, 2 * N + 1}};
    for (const auto& r : ranges) {
        const uint32_t first = r[0] < held - 1 ? r[0] : held - 1, count = r[1] < held - first ? r[1] : held - first;
        const size_t big = (size_t)k * N + 1;
        std::unique_ptr<uint64_t[]> rows(new uint64_t[count * big]);
        if (fhe::narrow_sample_extract(N, k, narrow.get(), held, bits, first, count, rows.get())) return 1;
        printf(" %016llx", (unsigned long long)checksum(rows.get(), count * big));
    }
    printf("\n");
    // the refusals touch nothing: null buffers would fault if they did
    if (!fhe::narrow_sample_extract(N, k, nullptr, held, bits, held, 1, nullptr)) return 1;
    if (!fhe::glwe_narrow(N, k, nullptr, held, 7, nullptr) || !fhe::glwe_widen(N, k, nullptr, held, 33, nullptr)) return 1;
    return 0;
}

int main() {
    const uint32_t shapes[4][2] = {{256, 1}, {256, 2}, {512, 3}, {2048, 1}};
    const uint32_t widths[6] = {8, 13, 16, 21, 31, 32};
    for (const auto& s : shapes)
        for (uint32_t bits : widths) {
            const uint32_t N = s[0], k = s[1];
            std::set<uint32_t> held = {1, N - 1, N, N + 1, 2 * N + 1};
            bool exact = false, short_one = false;
            for (uint32_t m = 2; m < N && !(exact && short_one); m++) {   // the last stream of N + m blocks has k N + m fields
                const uint64_t used = ((uint64_t)k * N + m) * bits;
                if (!exact && used % 64 == 0) { held.insert(N + m); exact = true; }
                if (!short_one && used % 64 == 63) { held.insert(N + m); short_one = true; }
            }
            if (!exact || short_one != (bits % 2 == 1)) return 2;
            for (uint32_t h : held)
                if (run(N, k, bits, h)) return 1;
        }
    return 0;
}
