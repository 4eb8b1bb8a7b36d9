// ks_mfma_launch.h -- the host side the matrix-core products share: the LWE keyswitch (Engine::launch_keyswitch,
// engine.hip), the packing keyswitch (Packing::pack_dev, packing_dev.hip) and the casting keys (CastKey::keyswitch_dev,
// cast_dev.hip), which run the LWE keyswitch's own product at another geometry.  Declared here, defined once, in engine.hip,
// next to the only inclusion of the two operand kernels (ks_mfma_prep_kernels.hip.h).
#pragma once
#include "device_buffer.h"
#include "ks_mfma_kernels.hip.h"

namespace fhe {

struct Engine;

// int8 matrix product on the matrix cores: digits -> A fragments, then 32x32x32 tiles over (samples, columns x planes, rows)
struct KsMfmaLaunch {
    uint32_t row_tiles, mt, gy;   // 32-sample tiles; of them per workgroup (64 mt threads); grid.y
    uint32_t chunks, spc;         // K chunks (grid.z), K steps per chunk
    size_t digit_bytes;           // A fragments of the batch
    dim3 grid(const KsMfmaGeom& g) const { return dim3(g.col_groups, gy, chunks); }
    void info(uint32_t out[5], uint32_t first, const KsMfmaGeom& g) const { out[0] = first; out[1] = mt; out[2] = chunks; out[3] = spc; out[4] = g.steps; }
};
KsMfmaLaunch ks_mfma_plan(const KsMfmaGeom& g, uint32_t count, uint32_t base_log, int cu_count, uint32_t chunks_override);
// The batch's digit fragments on stream s.  The buffer is zeroed when it is allocated and only grows: the pad slots stay
// zero, rows past the batch are never read.  One launch per span of the device's grid.y (grid_spans.h); reads the launches'
// error.  Another stream's launch may still read the allocation being replaced.
int ks_mfma_digits(Engine& e, DeviceBuffer<int8_t>& digits, const KsMfmaLaunch& l, const KsMfmaGeom& g, const uint64_t* d_lwes, uint32_t count, hipStream_t s);
// Only the buffer of the above, for a caller that writes the fragments with a kernel of its own (cast_dev.hip).
int ks_mfma_reserve_digits(Engine& e, DeviceBuffer<int8_t>& digits, const KsMfmaLaunch& l, hipStream_t s);
// keyswitch_mfma_kernel<l.mt> at l.grid(a.g) on stream s: the one place the product is instantiated and launched (the
// keyswitch and the casting keys).  Refuses a grid the device does not allow (Engine::one_span); otherwise only the launch:
// the caller reads hipGetLastError.
int ks_mfma_product(const Engine& e, const KsMfmaArgs& a, const KsMfmaLaunch& l, hipStream_t s);
// A key's words at d_std -> its balanced base-256 digit planes in B-fragment order at planes (col_groups x steps x 8 KB), on
// stream s, one launch per span of the device's grid.y.  Only the launches: the caller reads hipGetLastError and synchronises under its own name.
void ks_mfma_repack(const Engine& e, const uint64_t* d_std, int8_t* planes, const KsMfmaGeom& g, hipStream_t s);

}  // namespace fhe
