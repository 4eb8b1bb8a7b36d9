// grid_spans_main.cpp -- csrc/grid_spans.h on its own, for tests/test_grid_spans_host.py.  Arguments: COUNT,LIMIT pairs;
// for each, one line `COUNT LIMIT: spans=S per=P` followed by the spans as `first+count`, all of them up to 8 spans, else
// the first two, the last two and `...`; and after walking EVERY span one line `walk: ok` or `walk: <what is wrong>`: the
// spans must be consecutive from 0, each of 1 .. LIMIT indices, only the last shorter than per, and add up to COUNT.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../fhe-string-bounty_amd/csrc/grid_spans.h"

static const char* walk(const fhe::GridSpans& s, uint64_t count, uint32_t limit) {
    if (count == 0 || limit == 0) return s.spans == 0 ? nullptr : "spans where nothing can be launched";
    if (s.spans == 0) return "no span for a non-empty count";
    if (s.per == 0 || s.per > limit) return "per outside 1 .. limit";
    if (s.spans != (count + limit - 1) / limit) return "more launches than ceil(count / limit)";
    uint64_t next = 0;
    for (uint64_t i = 0; i < s.spans; i++) {
        const fhe::GridSpan g = s.at(i);
        if (g.first != next) return "a span does not start where the one before ended";
        if (g.count == 0 || g.count > limit) return "a span outside 1 .. limit";
        if (i + 1 < s.spans && g.count != s.per) return "a span before the last is not full";
        next += g.count;
    }
    return next == count ? nullptr : "the spans do not add up to the count";
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        char* comma = nullptr;
        const uint64_t count = strtoull(argv[a], &comma, 10);
        if (*comma != ',') { fprintf(stderr, "COUNT,LIMIT expected, got %s\n", argv[a]); return 2; }
        const uint32_t limit = (uint32_t)strtoul(comma + 1, nullptr, 10);
        const fhe::GridSpans s = fhe::grid_spans(count, limit);
        printf("%" PRIu64 " %u: spans=%" PRIu64 " per=%u", count, limit, s.spans, s.per);
        for (uint64_t i = 0; i < s.spans; i++) {
            if (s.spans > 8 && i == 2) { printf(" ..."); i = s.spans - 3; continue; }
            const fhe::GridSpan g = s.at(i);
            printf(" %" PRIu64 "+%u", g.first, g.count);
        }
        const char* why = walk(s, count, limit);
        printf("\nwalk: %s\n", why ? why : "ok");
    }
    return 0;
}
