// grid_spans.h -- the one piece of arithmetic behind every launch whose grid.y or grid.z grows with a batch or a key size:
// `count` indices under a device limit of `limit` per grid dimension (hipDeviceProp_t::maxGridSize, read once in
// Engine::create) -> consecutive spans of at most `limit` indices, one launch each.  A launch site either loops over the
// spans, passing span.first to the kernel (or offsetting its pointers by it), or -- where a documented batch limit keeps
// the dimension small -- asks for exactly one span and refuses otherwise (Engine::one_span).  Plain host C++, no HIP: it is
// compiled on its own into tests/grid_spans_main.cpp.
#pragma once
#include <stdint.h>

namespace fhe {

struct GridSpan {
    uint64_t first;    // first index of the span
    uint32_t count;    // 1 .. limit indices: the grid dimension of its launch
};

struct GridSpans {
    uint64_t count = 0;    // indices in all
    uint32_t per = 0;      // indices per span but the last (0: nothing to launch, or no launch possible)
    uint64_t spans = 0;    // launches: ceil(count / per)
    GridSpan at(uint64_t i) const {
        const uint64_t first = i * per, left = count - first;
        return GridSpan{first, (uint32_t)(left < per ? left : per)};
    }
};

// limit == 0 (a device that reports no grid in that dimension) or count == 0 -> no spans; the caller tells them apart by count.
inline GridSpans grid_spans(uint64_t count, uint32_t limit) {
    GridSpans s;
    s.count = count;
    if (count == 0 || limit == 0) return s;
    s.per = count < limit ? (uint32_t)count : limit;
    s.spans = count / s.per + (count % s.per != 0);
    return s;
}

}  // namespace fhe
