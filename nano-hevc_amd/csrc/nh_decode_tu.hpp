// nh_decode_tu.hpp -- argument blocks and small helpers of the config-4 closed-loop
// DECODER (nh_decode_tu.hip).  Nothing here is shared with
// the encoder's translation units: the coherent line-word accessors restate the
// few lines nh_intraloop.hip keeps for its own wavefronts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nh {

// One plane set, as every kernel of the decoder sees it.  Planes are numbered
// pl = g * ppg + c; the TU map and the pred-mode map hold tu_plane = (h/4)*(w/4)
// bytes per plane in that order.
struct TuSetDev {
    int64_t base, plane_stride, group_stride;   // in samples
    int64_t tu_plane;
    int32_t w, h, pitch, ppg;
    int32_t nplanes;
    int32_t rcols, rrows;   // 32x32 regions per plane row / column (stage R, pred map)
    int32_t aligned;        // 4-sample row pieces may be moved as one vector access
};

struct TuDecArgs {
    const uint8_t* tu;
    const uint8_t* pm;
    int16_t* rec;       // stage R's residual in, the reconstruction out
    int32_t* work;      // [0] ticket, [1] status, [2..3] pad, then the 64-bit line words
    TuSetDev s;
    int32_t crows, ccols;   // CTU rows / columns of a plane (the CTB size is the kernel's template argument)
    int32_t lw;         // line words per plane
};

constexpr int kTuDecSpinLimit = 1 << 20;   // polls before a wait counts as stalled; a legitimate wait is a few CTU steps
constexpr int kTuDecLines0 = 4;            // int32 words before the line words (8-B aligned)

__device__ __forceinline__ int tud_ld_sys(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Tagged line words cross XCDs: single-copy-atomic 64-bit accesses at system scope
// (write-through / coherent read, no L2 writeback or invalidate).
__device__ __forceinline__ uint64_t tud_ld_sys64(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void tud_st_sys64(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Map validity of one 4x4 unit: value v in [2, log2 ctb], the
// aligned n x n square (n = 1 << v) holding the unit inside the plane, every unit
// of that square equal to v.  The square's top-left unit walks the square; every
// other unit compares with it -- together: a partition into aligned dyadic squares.
__device__ __forceinline__ bool tu_unit_valid(const uint8_t* tu, int w4, int h4, int ux, int uy, int log2ctb) {
    const int v = tu[(int64_t)uy * w4 + ux];
    if (v < 2 || v > log2ctb) return false;
    const int nu = 1 << (v - 2), ox = ux & ~(nu - 1), oy = uy & ~(nu - 1);
    if (ox + nu > w4 || oy + nu > h4) return false;
    if (ox != ux || oy != uy) return tu[(int64_t)oy * w4 + ox] == v;
    for (int j = 0; j < nu; ++j)
        for (int i = 0; i < nu; ++i)
            if (tu[(int64_t)(oy + j) * w4 + ox + i] != v) return false;
    return true;
}

}  // namespace nh
