// nh_decode_tu.hip -- the config-4 closed-loop DECODER:
// TU map + pred-mode map + levels -> the reconstruction nh_tu_pipeline_planes_closed
// wrote, and the encoder-side post-pass that derives the pred-mode map.
//
//   k_tu_pred_map    (src, rec, tu) -> pm.  Every neighbour of a TU is a finished
//                    reconstruction sample, so every TU is independent of every
//                    other: no wavefront.  One 64-lane workgroup per 32x32 region,
//                    one lane per 4x4 unit; a TU's DC sum and its two residual
//                    energies (int64, int16-wrapping residual) are added up in LDS
//                    slots of the TU's top-left unit.
//   k_dequant_inv_tu stage R over a TU map, sizes 4 (DST / DCT), 8, 16, 32:
//                    res = inverse_transform(dequantize_block(level, qp)).astype(int16)
//                    in ring arithmetic mod 2^32 throughout (64-bit dequantiser
//                    product, wrapping 32-bit products and sums in both passes): exact
//                    for EVERY level value of the input dtype.  One 256-thread
//                    workgroup per 32x32 region, the matrix form of transform.py
//                    with the basis in LDS; a thread owns 4 neighbouring samples;
//                    the sums stop at the TU's last nonzero level row / column.
//   k_tu_check_map   the validity pre-pass: a bad map sets status 2.
//   k_tu_dec_closed  stage P, the CTU-row wavefront of §4.4a: rows claimed by ticket
//                    (row-major across planes), a CTU's bottom row handed down as
//                    tagged 64-bit line words, bounded poll.  Inside a CTU the TUs
//                    run in dataflow rounds (a TU is ready once the units above and
//                    left of it are done): lane = 4x4 unit, every ready TU of every
//                    size is predicted in the same round, 16 samples per lane.
//                    CTB 16: four planes per wave in lock-step, 16 lanes each.
// Every neighbour the wavefront reads is a clipped 8-bit sample or 128, so its
// prediction arithmetic never leaves int16; the pred map kernel takes any int16
// reconstruction and source and works in 32 bits (|sum| < 2^23).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include "nh_common.hpp"
#include "nh_internal.hpp"
#include "nh_decode_tu.hpp"

namespace nh {

typedef short v4s __attribute__((ext_vector_type(4)));
typedef int v4w __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int16_t* tud_plane(int16_t* p, const TuSetDev& s, int pl) {
    const int g = pl / s.ppg, c = pl - g * s.ppg;
    return p + s.base + (int64_t)g * s.group_stride + (int64_t)c * s.plane_stride;
}

__device__ __forceinline__ int tud_clamp_v(int v) { return v < 2 ? 2 : (v > 5 ? 5 : v); }

// The 32-point basis as bytes (|DCT32| <= 90), built at compile time; stage R copies it to LDS.
struct alignas(16) TuBasis32 {   // read as 32-bit words
    int8_t c[32][32];
};
constexpr TuBasis32 make_tu_basis32() {
    TuBasis32 b{};
    for (int k = 0; k < 32; ++k)
        for (int n = 0; n < 32; ++n) b.c[k][n] = (int8_t)dct32(k, n);
    return b;
}
__constant__ TuBasis32 c_tu_basis32 = make_tu_basis32();

// ---------------------------------------------------------------------------
// Pred-mode map: pm = 1 (DC) iff e_dc <= e_planar.
// A map value outside [2, 5] is clamped and a TU that crosses the plane edge
// reads clamped positions: any map is memory-safe, only a valid one meaningful.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_tu_pred_map(const int16_t* __restrict__ src, const int16_t* __restrict__ rec,
                                                    const uint8_t* __restrict__ tu, uint8_t* __restrict__ pm,
                                                    TuSetDev s) {
    __shared__ int dsum[64];
    __shared__ unsigned long long edc[64], epl[64];
    const int lane = threadIdx.x;
    const uint32_t rpp = (uint32_t)s.rcols * (uint32_t)s.rrows;
    const int pl = blockIdx.x / rpp, r = blockIdx.x - pl * rpp;
    const int ry = r / s.rcols, rx = r - ry * s.rcols;
    const int ux = lane & 7, uy = lane >> 3, x = rx * 32 + 4 * ux, y = ry * 32 + 4 * uy;
    const bool on = x < s.w && y < s.h;
    dsum[lane] = 0;
    edc[lane] = 0;
    epl[lane] = 0;
    __syncthreads();
    const int w4 = s.w / 4;
    const int16_t* sp = tud_plane(const_cast<int16_t*>(src), s, pl);
    const int16_t* rp = tud_plane(const_cast<int16_t*>(rec), s, pl);
    int v = 2, n = 4, tx = x, ty = y, own = lane;
    int top[4], left[4], tr = 128, bl = 128;
    if (on) {
        v = tud_clamp_v(tu[(int64_t)pl * s.tu_plane + (int64_t)(y / 4) * w4 + x / 4]);
        n = 1 << v;
        tx = x & ~(n - 1);
        ty = y & ~(n - 1);
        own = ((ty & 31) >> 2) * 8 + ((tx & 31) >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            top[i] = ty == 0 ? 128 : rp[(int64_t)(ty - 1) * s.pitch + x + i];
            left[i] = tx == 0 ? 128 : rp[(int64_t)(y + i) * s.pitch + tx - 1];
        }
        if (ty > 0) tr = rp[(int64_t)(ty - 1) * s.pitch + min(tx + n - 1, s.w - 1)];
        if (tx > 0) bl = rp[(int64_t)min(ty + n - 1, s.h - 1) * s.pitch + tx - 1];
        int part = 0;
        if (y == ty) part += top[0] + top[1] + top[2] + top[3];
        if (x == tx) part += left[0] + left[1] + left[2] + left[3];
        if (y == ty || x == tx) atomicAdd(&dsum[own], part);
    }
    __syncthreads();
    if (on) {
        const int dc = (dsum[own] + n) >> (v + 1);   // floor division by 2 n (intra.py:61)
        const int lx0 = x - tx, ly0 = y - ty;
        long long ed = 0, ep = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ly0 + j;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lx = lx0 + i;
                const int o = sp[(int64_t)(y + j) * s.pitch + x + i];
                const int p = ((n - 1 - lx) * left[j] + (lx + 1) * tr + (n - 1 - ly) * top[i] + (ly + 1) * bl + n) >> (v + 1);
                const int d0 = (int16_t)(uint16_t)(uint32_t)(o - dc), d1 = (int16_t)(uint16_t)(uint32_t)(o - (int)(int16_t)p);
                ed += (long long)(d0 * d0);   // |d| <= 2^15: the square fits 31 bits
                ep += (long long)(d1 * d1);
            }
        }
        atomicAdd(&edc[own], (unsigned long long)ed);
        atomicAdd(&epl[own], (unsigned long long)ep);
    }
    __syncthreads();
    if (on) pm[(int64_t)pl * s.tu_plane + (int64_t)(y / 4) * w4 + x / 4] = edc[own] <= epl[own] ? 1 : 0;   // DC wins ties
}

// ---------------------------------------------------------------------------
// Stage R over a TU map.
// ---------------------------------------------------------------------------
template <int LB, bool ALIGNED>
__global__ void __launch_bounds__(256) k_dequant_inv_tu(const void* __restrict__ lvl_v, int16_t* __restrict__ res,
                                                        const uint8_t* __restrict__ tu, TuSetDev s, int is_luma,
                                                        int scale, int per) {
    __shared__ int32_t A[32][33], B[32][33];
    __shared__ int32_t T32[32][33];   // T32[k][n] = DCT32[k][n]; DCT_N[k][n] = T32[k * 32 / N][n]
    __shared__ int32_t D4[4][4];
    __shared__ int rext[64], cext[64];   // per TU (slot of its top-left unit): rows / columns up to the last nonzero level
    __shared__ uint8_t vmap[64];
    const int t = threadIdx.x;
    const uint32_t rpp = (uint32_t)s.rcols * (uint32_t)s.rrows;
    const int pl = blockIdx.x / rpp, r = blockIdx.x - pl * rpp;
    const int ry = r / s.rcols, rx = r - ry * s.rcols;
    const int w4 = s.w / 4;
    {   // 4 basis bytes per thread
        const uint32_t q = reinterpret_cast<const uint32_t*>(&c_tu_basis32.c[0][0])[t];
#pragma unroll
        for (int i = 0; i < 4; ++i) T32[t >> 3][(t & 7) * 4 + i] = (int32_t)(int8_t)(q >> (8 * i));
    }
    if (t < 16) D4[t >> 2][t & 3] = dst4c(t >> 2, t & 3);
    if (t < 64) {
        const int x = rx * 32 + 4 * (t & 7), y = ry * 32 + 4 * (t >> 3);
        vmap[t] = (x < s.w && y < s.h) ? (uint8_t)tud_clamp_v(tu[(int64_t)pl * s.tu_plane + (int64_t)(y / 4) * w4 + x / 4]) : 2;
        rext[t] = 0;
        cext[t] = 0;
    }
    // this thread: row lr of the region, columns lc .. lc + 3 (one row of one 4x4 unit)
    const int lr = t >> 3, lc = (t & 7) * 4;
    const int x = rx * 32 + lc, y = ry * 32 + lr;
    const bool on = x < s.w && y < s.h;
    const int g = pl / s.ppg, c = pl - g * s.ppg;
    const int64_t off = s.base + (int64_t)g * s.group_stride + (int64_t)c * s.plane_stride + (int64_t)y * s.pitch + x;
    int32_t l[4] = {0, 0, 0, 0};
    if (on) {
        if constexpr (LB == 4) {
            const int32_t* p = static_cast<const int32_t*>(lvl_v) + off;
            if constexpr (ALIGNED) {
                const v4w q = *reinterpret_cast<const v4w*>(p);
                l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) l[i] = p[i];
            }
        } else {
            const int16_t* p = static_cast<const int16_t*>(lvl_v) + off;
            if constexpr (ALIGNED) {
                const v4s q = *reinterpret_cast<const v4s*>(p);
                l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) l[i] = p[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) A[lr][lc + i] = l[i] ? dequant_i32(l[i], scale, per) : 0;   // quant.py:112-123, int64 inside; 0 -> 0
    __syncthreads();
    const int v = vmap[(lr >> 2) * 8 + (lc >> 2)], n = 1 << v, step = 32 >> v;
    const int ty = lr & ~(n - 1), tx = lc & ~(n - 1);   // the TU's origin in the region
    const int li = lr - ty, lj = lc - tx;
    // A zero level dequantises to 0 and a zero coefficient adds nothing to either pass, so both
    // sums stop at the TU's last nonzero row / column: the same ring arithmetic minus zero terms
    // (pass 1 of an all-zero column is (0 + rnd) >> sh = 0: pass 2 never reads it).
    const int own = (ty >> 2) * 8 + (tx >> 2);
    {
        const int last = l[3] ? 4 : l[2] ? 3 : l[1] ? 2 : l[0] ? 1 : 0;
        if (last) {
            atomicMax(&rext[own], li + 1);
            atomicMax(&cext[own], lj + last);
        }
    }
    __syncthreads();
    const int re = rext[own], ce = cext[own];
    const bool dst = is_luma && n == 4;
    const int sh = v + 5;
    const uint32_t rnd = 1u << (sh - 1);
    {   // pass 1 (transform.py:221-227): temp[i][j] = (sum_k T[k][i] * c[k][j] + rnd) >> sh
        uint32_t acc[4] = {rnd, rnd, rnd, rnd};
        const int kn = lj < ce ? re : 0;
        for (int k = 0; k < kn; ++k) {
            const uint32_t cf = (uint32_t)(dst ? D4[k][li] : T32[k * step][li]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += cf * (uint32_t)A[ty + k][lc + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) B[lr][lc + i] = (int32_t)acc[i] >> sh;
    }
    __syncthreads();
    uint32_t acc[4] = {rnd, rnd, rnd, rnd};
    // pass 2 (transform.py:230-236): res[i][j] = (sum_k temp[i][k] * T[k][j] + rnd) >> sh
    for (int k = 0; k < ce; ++k) {
        const uint32_t b = (uint32_t)B[lr][tx + k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += b * (uint32_t)(dst ? D4[k][lj + i] : T32[k * step][lj + i]);
    }
    if (on) {
        int16_t o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (int16_t)(uint16_t)(uint32_t)((int32_t)acc[i] >> sh);   // astype(int16)
        int16_t* q = res + off;
        if constexpr (ALIGNED) {
            *reinterpret_cast<v4s*>(q) = v4s{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = o[i];
        }
    }
}

// ---------------------------------------------------------------------------
// Validity pre-pass: status 2 for a map that is no partition into aligned dyadic
// squares inside the plane, or for a pred mode other than 0 / 1.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tu_check_map(const uint8_t* __restrict__ tu, const uint8_t* __restrict__ pm,
                                                      TuSetDev s, int log2ctb, int32_t* status) {
    const int w4 = s.w / 4, h4 = s.h / 4;
    const int64_t total = s.tu_plane * s.nplanes;
    bool bad = false;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pl = i / s.tu_plane;
        const int u = (int)(i - pl * s.tu_plane), uy = u / w4, ux = u - uy * w4;
        bad |= !tu_unit_valid(tu + pl * s.tu_plane, w4, h4, ux, uy, log2ctb);
        bad |= pm[i] > 1;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicMax(status, 2);
}

// ---------------------------------------------------------------------------
// Stage P: the CTU-row wavefront.  CTU (cx, cy) needs (cx - 1, cy) -- the same
// wave, its right column kept in LDS -- and (cx, cy - 1): the bottom row of the
// CTU above, polled as tagged line words (tag = producing CTU row + 1; the word IS
// the flag, one coherent round trip per CTU).  A row overwrites a CTU's words only
// after reading them, and only the row below reads what it writes.  Tickets are
// claimed row-major across plane groups, so the row above was claimed earlier by a wave
// that runs or has finished: the wait always ends, for any number of resident waves.
// The launch follows the validity pre-pass on the stream: a flagged map returns
// here before any ticket is taken, so nothing ever waits on a bad map.
// ---------------------------------------------------------------------------
template <bool ALIGNED, int CTB>
__global__ void __launch_bounds__(64) k_tu_dec_closed(TuDecArgs a) {
    // CTB 32: one plane per wave, 64 units.  CTB 16: a CTU has 16 units, so a wave takes the same CTU
    // row of NPL = 4 consecutive planes in lock-step, 16 lanes each; the planes never exchange data.
    constexpr int U = CTB / 4, UU = U * U, NPL = 64 / UU, RS = CTB + 2;
    // per plane: [0][1..]: row above, [1..][0]: column left, [1 + y][1 + x]: the CTU
    __shared__ int16_t rcs[NPL][CTB + 1][RS];
    __shared__ int row_s, stall_s;
    if (tud_ld_sys(&a.work[1])) return;
    const int lane = threadIdx.x, q = lane / UU, u = lane % UU;   // plane of the wave, unit of the CTU
    const TuSetDev& s = a.s;
    constexpr int ctb = CTB;
    const int w4 = s.w / 4;
    int16_t (*rc)[RS] = rcs[q];
    uint64_t* lines = reinterpret_cast<uint64_t*>(a.work + kTuDecLines0);
    const int groups = (s.nplanes + NPL - 1) / NPL;
    const int total = a.crows * groups;
    for (;;) {
        if (lane == 0) {
            row_s = atomicAdd(&a.work[0], 1);
            stall_s = 0;
        }
        __syncthreads();
        const int tk = row_s;
        if (tk >= total) break;
        const int cy = tk / groups, plq = (tk - cy * groups) * NPL + q;
        const bool plane_on = plq < s.nplanes;   // the last group of a set may be short
        const int pl = plane_on ? plq : s.nplanes - 1;
        int16_t* rec = tud_plane(a.rec, s, pl);
        const uint8_t* tu = a.tu + (int64_t)pl * s.tu_plane;
        const uint8_t* pm = a.pm + (int64_t)pl * s.tu_plane;
        uint64_t* line = lines + (int64_t)pl * a.lw;
        const int y0c = cy * ctb;
        if (u < ctb) rc[1 + u][0] = 128;   // x == 0: left = 128 (block.py:45-50)
        const int ux = u % U, uy = u / U, y = y0c + 4 * uy;
        // this lane's unit of CTU cxn: map byte and residual (int16 pairs), 0 past the plane's edge
        auto fetch = [&](int cxn, int& vv, uint32_t (&pk)[8]) {
            const int xn = cxn * ctb + 4 * ux;
            vv = 2;
            if (plane_on && xn < s.w && y < s.h) {
                vv = tu[(int64_t)(y / 4) * w4 + xn / 4];
                const int16_t* q = rec + (int64_t)y * s.pitch + xn;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (ALIGNED) {
                        const uint2 d = *reinterpret_cast<const uint2*>(q + (int64_t)j * s.pitch);
                        pk[2 * j] = d.x;
                        pk[2 * j + 1] = d.y;
                    } else {
                        const int16_t* r = q + (int64_t)j * s.pitch;
                        pk[2 * j] = (uint32_t)(uint16_t)r[0] | ((uint32_t)(uint16_t)r[1] << 16);
                        pk[2 * j + 1] = (uint32_t)(uint16_t)r[2] | ((uint32_t)(uint16_t)r[3] << 16);
                    }
                }
            }
        };
        int v_n = 2;
        uint32_t pk_n[8] = {};
        fetch(0, v_n, pk_n);
        for (int cx = 0; cx < a.ccols; ++cx) {
            const int x0c = cx * ctb;
            const int x = x0c + 4 * ux;
            const bool on = plane_on && x < s.w && y < s.h;
            int nu = 1, ox = ux, oy = uy, dc_mode = 0;
            int val[16];
            int16_t* p = rec + (int64_t)y * s.pitch + x;
            uint64_t dep = 0;   // the units right above and left of this lane's TU
            if (on) {
                nu = 1 << (v_n - 2);
                ox = ux & ~(nu - 1);
                oy = uy & ~(nu - 1);
                dc_mode = pm[(int64_t)(y0c / 4 + oy) * w4 + x0c / 4 + ox];
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    val[2 * m] = (int)(int16_t)(uint16_t)(pk_n[m] & 0xffffu);
                    val[2 * m + 1] = (int)pk_n[m] >> 16;
                }
                for (int k = 0; k < nu; ++k) {
                    if (oy > 0) dep |= 1ull << (q * UU + (oy - 1) * U + ox + k);
                    if (ox > 0) dep |= 1ull << (q * UU + (oy + k) * U + ox - 1);
                }
            }
            // the next CTU's map byte and residual: in flight under this CTU's wait and rounds
            if (cx + 1 < a.ccols) fetch(cx + 1, v_n, pk_n);
            // top row of this CTU: 128 at y == 0, else the CTU above's bottom row
            if (cy == 0) {
                if (u < ctb) rc[0][1 + u] = 128;
            } else {
                const int nw = min(ctb, s.w - x0c) / 2;
                const bool need = plane_on && u < nw;
                uint32_t wv = 0;
                int spins = 0;
                for (;;) {
                    bool ok = true;
                    if (need) {
                        const uint64_t q = tud_ld_sys64(line + x0c / 2 + u);
                        ok = (int)(q >> 32) == cy;
                        wv = (uint32_t)q;
                    }
                    if (__builtin_amdgcn_read_exec() == __ballot(ok)) break;
                    __builtin_amdgcn_s_sleep(1);
                    ++spins;
                    if (spins > kTuDecSpinLimit || ((spins & 1023) == 0 && tud_ld_sys(&a.work[1]))) {
                        if (lane == 0) atomicMax(&a.work[1], 1);
                        stall_s = 1;
                        break;
                    }
                }
                if (need) {
                    rc[0][1 + 2 * u] = (int16_t)(wv & 0xffffu);
                    rc[0][2 + 2 * u] = (int16_t)(wv >> 16);
                }
            }
            __syncthreads();
            if (stall_s) break;
            const int n = 4 * nu, lg = 31 - __clz(n);
            const int px = 4 * ox, py = 4 * oy;        // the TU's origin in the CTU
            const int lx0 = 4 * (ux - ox), ly0 = 4 * (uy - oy);
            bool pending = on;
            // a valid map's first pending TU in z-order is always ready: every round finishes one
            for (int round = 0; round < UU; ++round) {
                const uint64_t todo = __ballot(pending);   // bit = q * UU + uy * U + ux
                if (!todo) break;
                const bool ready = pending && !(dep & todo);
                if (ready) {
                    if (dc_mode) {   // intra.py:46-62
                        int sum = n;
                        for (int k = 0; k < n; ++k) sum += rc[py][1 + px + k] + rc[1 + py + k][px];
                        const int dc = sum >> (lg + 1);
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int r = (int)(int16_t)(uint16_t)(uint32_t)(dc + val[q]);   // reconstruct_block: int16 wrap
                            val[q] = min(255, max(0, r));
                        }
                    } else {         // planar, tr = top[-1], bl = left[-1] (intra.py:81-113)
                        const int tr = rc[py][px + n], bl = rc[py + n][px];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int ly = ly0 + j, lf = rc[1 + py + ly][px];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int lx = lx0 + i, tp = rc[py][1 + px + lx];
                                const int pr = ((n - 1 - lx) * lf + (lx + 1) * tr + (n - 1 - ly) * tp + (ly + 1) * bl + n) >> (lg + 1);
                                const int r = (int)(int16_t)(uint16_t)(uint32_t)(pr + val[4 * j + i]);
                                val[4 * j + i] = min(255, max(0, r));
                            }
                        }
                    }
                }
                // every ready TU has read its neighbours (none of them is a TU of this round)
                __syncthreads();
                if (ready) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i) rc[1 + 4 * uy + j][1 + 4 * ux + i] = (int16_t)val[4 * j + i];
                    pending = false;
                }
                __syncthreads();
            }
            // publish the bottom row first (the next CTU row polls it), then store the CTU
            if (cy + 1 < a.crows) {
                const int nw = min(ctb, s.w - x0c) / 2;
                if (plane_on && u < nw) {
                    const uint32_t lo = (uint16_t)rc[ctb][1 + 2 * u], hi = (uint16_t)rc[ctb][2 + 2 * u];
                    tud_st_sys64(line + x0c / 2 + u, ((uint64_t)(uint32_t)(cy + 1) << 32) | lo | (hi << 16));
                }
            }
            if (on) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (ALIGNED) {
                        *reinterpret_cast<v4s*>(p + (int64_t)j * s.pitch) =
                            v4s{(short)val[4 * j], (short)val[4 * j + 1], (short)val[4 * j + 2], (short)val[4 * j + 3]};
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) p[(int64_t)j * s.pitch + i] = (int16_t)val[4 * j + i];
                    }
                }
            }
            // slide: this CTU's right column is the next one's left column
            int16_t keep = 0;
            if (u < ctb) keep = rc[1 + u][ctb];
            __syncthreads();
            if (u < ctb) rc[1 + u][0] = keep;
        }
        __syncthreads();
        if (stall_s) break;
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static int tud_layout(const nh_plane_set* set, int ctb, TuSetDev& d, const char* who) {
    if (!set) {
        set_error(std::string(who) + ": null argument");
        return NH_EARG;
    }
    if (ctb != 16 && ctb != 32) {
        set_error(std::string(who) + ": ctb must be 16 or 32");
        return NH_EARG;
    }
    if ((set->width & 3) || (set->height & 3)) {
        set_error(std::string(who) + ": width and height must be multiples of 4");
        return NH_EARG;
    }
    if (set->width < 4 || set->height < 4 || set->width > 65532 || set->height > 65532 || set->pitch < set->width ||
        set->planes_per_group < 1 || set->num_groups < 0) {
        set_error(std::string(who) + ": plane set must have sizes in 4..65532, pitch >= width, >= 1 plane per group");
        return NH_EARG;
    }
    const int64_t np = (int64_t)set->planes_per_group * set->num_groups;
    d.base = set->base;
    d.plane_stride = set->plane_stride;
    d.group_stride = set->group_stride;
    d.tu_plane = (int64_t)(set->height / 4) * (set->width / 4);
    d.w = set->width;
    d.h = set->height;
    d.pitch = set->pitch;
    d.ppg = set->planes_per_group;
    d.rcols = (set->width + 31) / 32;
    d.rrows = (set->height + 31) / 32;
    const int64_t crows = (set->height + ctb - 1) / ctb;
    if (np * d.rcols * d.rrows >= (1ll << 31) || np * crows >= (1ll << 30) || np * d.tu_plane >= (1ll << 40)) {
        set_error(std::string(who) + ": too many planes (>= 2^31 regions or >= 2^30 CTU rows)");
        return NH_EARG;
    }
    d.nplanes = (int32_t)np;
    d.aligned = !((set->base | set->plane_stride | set->group_stride | set->pitch) & 3);
    return NH_OK;
}

static int64_t tud_line_words(const nh_plane_set* set) { return (set->width / 2 + 1) & ~1ll; }   // 16-B multiples

}  // namespace nh

using namespace nh;

extern "C" int nh_tu_closed_pred_map(const int16_t* d_src, const int16_t* d_recon, const uint8_t* d_tu,
                                     const nh_plane_set* set, int ctb, uint8_t* d_pm, void* stream) {
    if (!d_src || !d_recon || !d_tu || !d_pm || !set) {
        set_error("nh_tu_closed_pred_map: null argument");
        return NH_EARG;
    }
    TuSetDev d{};
    NH_TRY(tud_layout(set, ctb, d, "nh_tu_closed_pred_map"));
    if (((uintptr_t)d_src | (uintptr_t)d_recon) & 1) {
        set_error("nh_tu_closed_pred_map: buffers must be aligned to their element size");
        return NH_EARG;
    }
    if (!d.nplanes) return NH_OK;
    k_tu_pred_map<<<(unsigned)((int64_t)d.nplanes * d.rcols * d.rrows), 64, 0, as_stream(stream)>>>(d_src, d_recon, d_tu,
                                                                                                 d_pm, d);
    NH_HIP(hipGetLastError());
    return NH_OK;
}

extern "C" int nh_dequant_inv_tu_planes(const void* d_lvl, int lvl_bytes, int16_t* d_res, const uint8_t* d_tu,
                                        const nh_plane_set* set, int ctb, int is_luma, int qp, void* stream) {
    if (!d_lvl || !d_res || !d_tu || !set) {
        set_error("nh_dequant_inv_tu_planes: null argument");
        return NH_EARG;
    }
    if (lvl_bytes != 2 && lvl_bytes != 4) {
        set_error("nh_dequant_inv_tu_planes: lvl_bytes must be 2 (int16) or 4 (int32)");
        return NH_EARG;
    }
    TuSetDev d{};
    NH_TRY(tud_layout(set, ctb, d, "nh_dequant_inv_tu_planes"));
    if (((uintptr_t)d_lvl & (uintptr_t)(lvl_bytes - 1)) || ((uintptr_t)d_res & 1)) {
        set_error("nh_dequant_inv_tu_planes: buffers must be aligned to their element size");
        return NH_EARG;
    }
    if (!d.nplanes) return NH_OK;
    const bool aligned = d.aligned && !((uintptr_t)d_lvl & (uintptr_t)(4 * lvl_bytes - 1)) && !((uintptr_t)d_res & 7);
    const int q = qp < 0 ? 0 : (qp > 51 ? 51 : qp);   // quant.py:35
    const int scale = dequant_scale(q % 6), per = q / 6;
    const unsigned grid = (unsigned)((int64_t)d.nplanes * d.rcols * d.rrows);
    hipStream_t s = as_stream(stream);
    const int luma = is_luma ? 1 : 0;
    if (lvl_bytes == 4) {
        if (aligned) k_dequant_inv_tu<4, true><<<grid, 256, 0, s>>>(d_lvl, d_res, d_tu, d, luma, scale, per);
        else k_dequant_inv_tu<4, false><<<grid, 256, 0, s>>>(d_lvl, d_res, d_tu, d, luma, scale, per);
    } else {
        if (aligned) k_dequant_inv_tu<2, true><<<grid, 256, 0, s>>>(d_lvl, d_res, d_tu, d, luma, scale, per);
        else k_dequant_inv_tu<2, false><<<grid, 256, 0, s>>>(d_lvl, d_res, d_tu, d, luma, scale, per);
    }
    NH_HIP(hipGetLastError());
    return NH_OK;
}

extern "C" int64_t nh_tu_decode_closed_workspace_bytes(const nh_plane_set* set, int ctb) {
    TuSetDev d{};
    if (tud_layout(set, ctb, d, "nh_tu_decode_closed_workspace_bytes")) return -1;
    return 4ll * kTuDecLines0 + 8ll * tud_line_words(set) * d.nplanes;
}

extern "C" int nh_tu_decode_planes_closed(const uint8_t* d_tu, const uint8_t* d_pm, const int32_t* d_lvl,
                                          const nh_plane_set* set, int ctb, int is_luma, int qp, int16_t* d_recon,
                                          void* d_work, void* stream) {
    if (!d_tu || !d_pm || !d_lvl || !d_recon || !d_work || !set) {
        set_error("nh_tu_decode_planes_closed: null argument");
        return NH_EARG;
    }
    TuDecArgs a{};
    NH_TRY(tud_layout(set, ctb, a.s, "nh_tu_decode_planes_closed"));
    if ((uintptr_t)d_work & 7) {
        set_error("nh_tu_decode_planes_closed: workspace must be 8-byte aligned");
        return NH_EARG;
    }
    if (((uintptr_t)d_lvl & 3) || ((uintptr_t)d_recon & 1)) {
        set_error("nh_tu_decode_planes_closed: buffers must be aligned to their element size");
        return NH_EARG;
    }
    hipStream_t s = as_stream(stream);
    a.lw = (int32_t)tud_line_words(set);
    NH_HIP(hipMemsetAsync(d_work, 0, 4ull * kTuDecLines0 + 8ull * a.lw * a.s.nplanes, s));
    if (!a.s.nplanes) return NH_OK;
    // stage R: every TU's residual into d_recon; a TU's residual is read from, and its
    // reconstruction written to, the same place by the same lane of the wavefront
    NH_TRY(nh_dequant_inv_tu_planes(d_lvl, 4, d_recon, d_tu, set, ctb, is_luma, qp, stream));
    const int64_t units = a.s.tu_plane * a.s.nplanes;
    k_tu_check_map<<<(unsigned)std::min<int64_t>(2048, (units + 255) / 256), 256, 0, s>>>(d_tu, d_pm, a.s,
                                                                                         ctb == 32 ? 5 : 4,
                                                                                         (int32_t*)d_work + 1);
    a.tu = d_tu;
    a.pm = d_pm;
    a.rec = d_recon;
    a.work = (int32_t*)d_work;
    a.crows = (set->height + ctb - 1) / ctb;
    a.ccols = (set->width + ctb - 1) / ctb;
    const bool aligned = a.s.aligned && !((uintptr_t)d_recon & 7);
    void (*kern)(TuDecArgs) = ctb == 32 ? (aligned ? k_tu_dec_closed<true, 32> : k_tu_dec_closed<false, 32>)
                                        : (aligned ? k_tu_dec_closed<true, 16> : k_tu_dec_closed<false, 16>);
    const int npl = ctb == 32 ? 1 : 4;   // planes per wave (k_tu_dec_closed)
    // persistent waves: one per CTU row of a plane group, capped at what can be resident
    int cus = 0, per_cu = 0;
    NH_TRY(device_cus(&cus));
    NH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64, 0));
    const int64_t rows = (int64_t)a.crows * ((a.s.nplanes + npl - 1) / npl), cap = (int64_t)std::max(1, per_cu) * cus;
    kern<<<(unsigned)(rows < cap ? rows : cap), 64, 0, s>>>(a);
    NH_HIP(hipGetLastError());
    return NH_OK;
}
