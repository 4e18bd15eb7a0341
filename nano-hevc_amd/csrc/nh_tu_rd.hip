// nh_tu_rd.hip -- config 4 with a CHOSEN or a SUPPLIED quadtree, open loop
// (DESIGN.md §3.4a, §4.4d).
//
//   k_tu_rd<true>   the TU-size search: per 32x32 region of a plane (one CTB 32, or
//                   four CTB 16) every aligned candidate TU of every size 4 .. ctb runs
//                   §3.4's chain, cost J = D + lambda * R (int64), and the quadtree is
//                   decided bottom-up: a node becomes one TU iff J_node <= the sum of
//                   its four best children (the parent wins ties; a node that overhangs
//                   the plane must split).
//   k_tu_rd<false>  the map-driven encode: the same chains, a candidate runs iff the
//                   caller's map holds a TU of that size there, and every candidate wins.
//   k_tu_rd_check   the validity pre-pass of the map-driven form (tu_unit_valid,
//                   DESIGN.md §3.10): a bad map sets the status word to 2 and the
//                   encode kernel returns before it reads anything else.
//
// One 256-thread workgroup per region.  The region, the source row above it and the
// column left of it are loaded once (open loop: every neighbour is a source sample,
// 128 outside the plane), so every candidate is independent of every other.  The
// four sizes run CONCURRENTLY, one wave each (CTB 32: wave 0 the 32x32 candidate on
// 32 lanes, wave 1 the four 16x16, wave 2 the sixteen 8x8 in two rounds, wave 3 the
// sixty-four 4x4 in four rounds): a candidate TU takes N lanes of its wave (lane t =
// column t, then row t), so the transposes between the 1-D passes need wave-level
// ordering only, and the 32-point chain on 32 lanes bounds the workgroup's time.
// The arithmetic is k_tu_process's (nh_intraloop.hip) with the same header
// primitives.  LDS holds one candidate image per size (levels, and the
// reconstruction in the transpose tile) with D / R per candidate; after one
// workgroup barrier the quadtree is decided size by size and every 4-sample row
// piece is stored once from the image of the largest winning node over it: levels,
// recon, tu and pm go to global memory once, in whole rows; the per-plane totals by
// 64-bit atomicAdd (integer sums: order-independent).  No workgroup waits on another.
//
// Multiplies are 24-bit (v_mad_i32_i24), exact for any int16 source by the argument
// at k_tu_process: the residual is int16 (forward operands < 2^21), dequantised
// coefficients are < 2^19, and the inverse pass-2 operands are a >> S of an int32
// sum bounded by 2^27, so < 2^21.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include "nh_common.hpp"
#include "nh_internal.hpp"
#include "nh_decode_tu.hpp"

namespace nh {

typedef short rd_v4s __attribute__((ext_vector_type(4)));
typedef int rd_v4w __attribute__((ext_vector_type(4)));

constexpr int kRdStatsPerPlane = 3;   // sum J, sum D, sum R
constexpr int kRdWorkWords = 4;       // [1] the status word (read with nh_intra_rdo_closed_status)

struct TuRdArgs {
    const int16_t* src;
    int32_t* lvl;
    int16_t* rec;
    uint8_t* tu;          // search: out; map-driven: in
    uint8_t* pm;
    unsigned long long* stats;
    const int32_t* work;  // map-driven only
    TuSetDev s;
    QuantParams q[4];     // per log2 size - 2
    int64_t lam;
    int32_t dqs, dq_per;
    int32_t log2ctb, is_luma;
};

// Nodes of a 32x32 region, all sizes in one index space: the (32 / N)^2 nodes of
// size N in raster order from rd_off(N).
constexpr int kRdNodes = 64 + 16 + 4 + 1;
__host__ __device__ constexpr int rd_off(int n) { return n == 4 ? 0 : n == 8 ? 64 : n == 16 ? 80 : 84; }

// Per-region LDS state.  Rows are padded: a TU's lanes walk a column of rows.
struct RdLds {
    int16_t S[33][34];          // [0][1 + x]: row above, [1 + y][0]: column left, [1 + y][1 + x]: the region
    int32_t tile[4][32][33];    // per size: the transpose tile; at the end the candidate recon as int16 pairs
    int32_t clvl[4][32][33];    // per size: the candidate levels
    long long cD[kRdNodes], bD[kRdNodes];   // candidate / best-so-far distortion per node
    int32_t cR[kRdNodes], bR[kRdNodes];
    uint8_t cact[kRdNodes], cpm[kRdNodes], win[kRdNodes];
    uint8_t vmap[64];
};

__device__ __forceinline__ int32_t rd_wrap16(int32_t v) { return (int16_t)(uint16_t)(uint32_t)v; }

// Orders one wave's LDS accesses: a wave's DS operations execute in order, so what
// any lane wrote before this point is what any lane of the same wave reads after it.
__device__ __forceinline__ void rd_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sums over the N lanes of an aligned group of one wave (every lane of the group active).
template <int N>
__device__ __forceinline__ int rd_sum(int v) {
#pragma unroll
    for (int m = N / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <int N>
__device__ __forceinline__ long long rd_sum64(long long v) {
#pragma unroll
    for (int m = N / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Every candidate of size N of the region, on ONE wave (all 64 lanes call; N lanes per TU).
template <int N, bool DST, bool SEARCH>
__device__ __forceinline__ void rd_chains(RdLds& L, const TuRdArgs& a, int x0, int y0, int lane) {
    constexpr int L2 = Log2<N>::v, S = L2 + 5, B = 32 / N, K = L2 - 2;
    constexpr int ROUNDS = (B * B * N + 63) / 64;
    const ChainQ cq = make_chainq(a.q[K], a.dqs, a.dq_per);
    int32_t (*tile)[33] = L.tile[K];
    int32_t (*clvl)[33] = L.clvl[K];
    for (int rnd = 0; rnd < ROUNDS; ++rnd) {
        const int vt = rnd * 64 + lane;
        const int g = vt / N, t = vt % N;
        const bool cand = g < B * B;
        const int tx = cand ? (g % B) * N : 0, ty = cand ? (g / B) * N : 0;   // the TU's origin in the region
        bool act = cand && x0 + tx + N <= a.s.w && y0 + ty + N <= a.s.h;    // wholly inside the plane
        if (!SEARCH) act = act && L.vmap[(ty >> 2) * 8 + (tx >> 2)] == L2;
        if (cand && t == 0) L.cact[rd_off(N) + g] = act ? 1 : 0;
        if (!__any(act)) continue;   // wave-uniform
        int32_t dc = 0, tr = 0, bl = 0;
        bool use_dc = true;
        if (act) {   // DC (intra.py:46-62) vs planar with tr = top[-1], bl = left[-1] (intra.py:81-113)
            dc = (rd_sum<N>((int)L.S[ty][1 + tx + t] + (int)L.S[1 + ty + t][tx]) + N) >> (L2 + 1);
            tr = L.S[ty][tx + N];
            bl = L.S[ty + N][tx];
            const int32_t tp = L.S[ty][1 + tx + t];
            long long ed = 0, ep = 0;
            for (int y = 0; y < N; ++y) {
                const int32_t o = L.S[1 + ty + y][1 + tx + t];
                const int32_t pl = ((N - 1 - t) * (int32_t)L.S[1 + ty + y][tx] + (t + 1) * tr + (N - 1 - y) * tp + (y + 1) * bl + N) >>
                                   (L2 + 1);
                const int32_t d1 = rd_wrap16(o - dc), d2 = rd_wrap16(o - pl);
                ed += (long long)(d1 * d1);   // |d| <= 2^15: the square fits 31 bits
                ep += (long long)(d2 * d2);
            }
            use_dc = rd_sum64<N>(ed) <= rd_sum64<N>(ep);   // DC wins ties
        }
        auto pred_at = [&](int y, int x) -> int32_t {
            if (use_dc) return dc;
            return ((N - 1 - x) * (int32_t)L.S[1 + ty + y][tx] + (x + 1) * tr + (N - 1 - y) * (int32_t)L.S[ty][1 + tx + x] +
                    (y + 1) * bl + N) >> (L2 + 1);
        };
        uint32_t v[N], r[N];
        if (act) {   // forward pass 1 on column t of the residual
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (uint32_t)rd_wrap16((int32_t)L.S[1 + ty + k][1 + tx + t] - pred_at(k, t));
            fwd1d<N, DST, Mul24>(v, r);
#pragma unroll
            for (int i = 0; i < N; ++i) tile[ty + i][tx + t] = rshift_round<S>(r[i]);
        }
        rd_wave_sync();
        int nz = 0;
        if (act) {   // forward pass 2 on row t, quant, dequant (row t is this lane's alone)
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[ty + t][tx + k];
            fwd1d<N, DST, Mul24>(v, r);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int32_t l = quant_s(rshift_round<S>(r[j]), cq.qs, cq.h_v, cq.hneg_v);
                clvl[ty + t][tx + j] = l;
                nz += l != 0;
                tile[ty + t][tx + j] = dequant_s(l, cq);
            }
        }
        rd_wave_sync();
        if (act) {   // inverse pass 1 on column t (column t is this lane's alone)
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[ty + k][tx + t];
            inv1d<N, DST, Mul24>(v, r);
#pragma unroll
            for (int i = 0; i < N; ++i) tile[ty + i][tx + t] = rshift_round<S>(r[i]);
        }
        rd_wave_sync();
        if (act) {   // inverse pass 2 on row t, reconstruct + clip, distortion
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[ty + t][tx + k];
            inv1d<N, DST, Mul24>(v, r);
            long long dd = 0;
#pragma unroll
            for (int j = 0; j < N; j += 2) {
                int32_t rc2[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int32_t rr = rd_wrap16(rshift_round<S>(r[j + q]));
                    const int32_t rc = rd_wrap16(pred_at(t, j + q) + rr);
                    rc2[q] = rc < 0 ? 0 : (rc > 255 ? 255 : rc);
                    const int32_t d = rd_wrap16((int32_t)L.S[1 + ty + t][1 + tx + j + q] - rc2[q]);
                    dd += (long long)(d * d);
                }
                // the row's recon as int16 pairs in the first N / 2 words of its tile row (read out above)
                tile[ty + t][tx + (j >> 1)] = (int32_t)((uint32_t)rc2[0] | ((uint32_t)rc2[1] << 16));
            }
            dd = rd_sum64<N>(dd);
            const int rate = rd_sum<N>(nz) + 1;   // + 1: the TU's own flag
            if (t == 0) {
                L.cD[rd_off(N) + g] = dd;
                L.cR[rd_off(N) + g] = rate;
                L.cpm[rd_off(N) + g] = use_dc ? 1 : 0;
            }
        }
    }
}

// The decision of every node of size N (one thread each), after the children's.
template <int N, bool SEARCH>
__device__ __forceinline__ void rd_decide(RdLds& L, const TuRdArgs& a) {
    constexpr int B = 32 / N;
    const int tid = threadIdx.x;
    if (tid < B * B) {
        const int n = rd_off(N) + tid;
        long long kd = 0;
        int32_t kr = 0;
        if constexpr (N > 4) {
            const int c = rd_off(N / 2) + (2 * (tid / B)) * (2 * B) + 2 * (tid % B);   // the first child
            kd = L.bD[c] + L.bD[c + 1] + L.bD[c + 2 * B] + L.bD[c + 2 * B + 1];
            kr = L.bR[c] + L.bR[c + 1] + L.bR[c + 2 * B] + L.bR[c + 2 * B + 1];
        }
        bool w = L.cact[n] != 0;
        if (SEARCH && N > 4 && w) w = L.cD[n] + a.lam * L.cR[n] <= kd + a.lam * kr;   // the parent wins ties
        L.bD[n] = w ? L.cD[n] : kd;
        L.bR[n] = w ? L.cR[n] : kr;
        L.win[n] = w ? 1 : 0;
    }
    __syncthreads();
}

template <bool SEARCH>
__global__ void __launch_bounds__(256) k_tu_rd(TuRdArgs a) {
    __shared__ RdLds L;
    if (!SEARCH && __hip_atomic_load(&a.work[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // a bad map
    const TuSetDev& s = a.s;
    const int tid = threadIdx.x;
    const uint32_t rpp = (uint32_t)s.rcols * (uint32_t)s.rrows;
    const int pl = blockIdx.x / rpp, rg = blockIdx.x - pl * rpp;
    const int ry = rg / s.rcols, rx = rg - ry * s.rcols;
    const int x0 = rx * 32, y0 = ry * 32;
    const int g = pl / s.ppg, c = pl - g * s.ppg;
    const int64_t poff = s.base + (int64_t)g * s.group_stride + (int64_t)c * s.plane_stride;
    const int16_t* sp = a.src + poff;
    const int w4 = s.w / 4;
    // this thread's row piece: row lr of the region, 4 samples from column lc (w, h multiples of 4)
    const int lr = tid >> 3, lc = (tid & 7) * 4;
    const bool on = x0 + lc < s.w && y0 + lr < s.h;
    const int64_t off = poff + (int64_t)(y0 + lr) * s.pitch + x0 + lc;
    {
        int16_t o[4] = {0, 0, 0, 0};
        if (on) {
            if (s.aligned) {
                const rd_v4s q = *reinterpret_cast<const rd_v4s*>(a.src + off);
                o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = a.src[off + i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) L.S[1 + lr][1 + lc + i] = o[i];
    }
    if (tid < 32) {          // the row above: 128 outside the plane (block.py:38-50)
        int16_t v = 128;
        if (y0 > 0) v = x0 + tid < s.w ? sp[(int64_t)(y0 - 1) * s.pitch + x0 + tid] : (int16_t)0;
        L.S[0][1 + tid] = v;
    } else if (tid < 64) {   // the column to the left
        const int k = tid - 32;
        int16_t v = 128;
        if (x0 > 0) v = y0 + k < s.h ? sp[(int64_t)(y0 + k) * s.pitch + x0 - 1] : (int16_t)0;
        L.S[1 + k][0] = v;
    } else if (tid < 128) {
        const int k = tid - 64;
        uint8_t v = 0;   // no TU
        if (!SEARCH) {
            const int x = x0 + 4 * (k & 7), y = y0 + 4 * (k >> 3);
            if (x < s.w && y < s.h) {   // clamped before anything indexes by it
                const int m = a.tu[(int64_t)pl * s.tu_plane + (int64_t)(y / 4) * w4 + x / 4];
                v = (uint8_t)(m < 2 ? 2 : (m > a.log2ctb ? a.log2ctb : m));
            }
        }
        L.vmap[k] = v;
    }
    __syncthreads();
    {   // one size per wave, the largest first; CTB 16 leaves wave 3 idle
        const int lane = tid & 63, size = a.log2ctb - (tid >> 6);   // wave-uniform
        if (size == 5) rd_chains<32, false, SEARCH>(L, a, x0, y0, lane);
        else if (size == 4) rd_chains<16, false, SEARCH>(L, a, x0, y0, lane);
        else if (size == 3) rd_chains<8, false, SEARCH>(L, a, x0, y0, lane);
        else if (size == 2) {
            if (a.is_luma) rd_chains<4, true, SEARCH>(L, a, x0, y0, lane);
            else rd_chains<4, false, SEARCH>(L, a, x0, y0, lane);
        }
    }
    __syncthreads();
    rd_decide<4, SEARCH>(L, a);
    rd_decide<8, SEARCH>(L, a);
    rd_decide<16, SEARCH>(L, a);
    if (a.log2ctb == 5) rd_decide<32, SEARCH>(L, a);
    // outputs, once, in whole rows: each row piece from the image of the largest winning node over it
    int k = -1, node = 0;
    for (int l2 = a.log2ctb; l2 >= 2 && k < 0; --l2) {
        const int n = rd_off(1 << l2) + (lr >> l2) * (32 >> l2) + (lc >> l2);
        if (L.win[n]) {
            k = l2 - 2;
            node = n;
        }
    }
    if (on && k >= 0) {
        const int32_t(*cl)[33] = L.clvl[k];
        const int n = 4 << k, tx = lc & ~(n - 1);
        const int32_t* rw = &L.tile[k][lr][tx + ((lc - tx) >> 1)];
        const uint32_t r0 = (uint32_t)rw[0], r1 = (uint32_t)rw[1];
        if (s.aligned) {
            *reinterpret_cast<rd_v4w*>(a.lvl + off) = rd_v4w{cl[lr][lc], cl[lr][lc + 1], cl[lr][lc + 2], cl[lr][lc + 3]};
            *reinterpret_cast<uint2*>(a.rec + off) = uint2{r0, r1};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) a.lvl[off + i] = cl[lr][lc + i];
            a.rec[off] = (int16_t)(r0 & 0xffffu);
            a.rec[off + 1] = (int16_t)(r0 >> 16);
            a.rec[off + 2] = (int16_t)(r1 & 0xffffu);
            a.rec[off + 3] = (int16_t)(r1 >> 16);
        }
        if (!(lr & 3)) {   // the unit's first row writes its map bytes
            const int64_t m = (int64_t)pl * s.tu_plane + (int64_t)((y0 + lr) / 4) * w4 + (x0 + lc) / 4;
            if (SEARCH) a.tu[m] = (uint8_t)(k + 2);
            a.pm[m] = L.cpm[node];
        }
    }
    if (tid == 0) {   // the CTB roots of the region: one 32x32 node or four 16x16 nodes
        long long d, r;
        if (a.log2ctb == 5) {
            d = L.bD[rd_off(32)];
            r = L.bR[rd_off(32)];
        } else {
            d = L.bD[80] + L.bD[81] + L.bD[82] + L.bD[83];
            r = (long long)L.bR[80] + L.bR[81] + L.bR[82] + L.bR[83];
        }
        unsigned long long* st = a.stats + (int64_t)pl * kRdStatsPerPlane;
        atomicAdd(st, (unsigned long long)(d + a.lam * r));
        atomicAdd(st + 1, (unsigned long long)d);
        atomicAdd(st + 2, (unsigned long long)r);
    }
}

// Validity pre-pass of the map-driven encode: status 2 for a map that is no
// partition of every plane into aligned squares of 4 .. ctb samples inside it.
__global__ void __launch_bounds__(256) k_tu_rd_check(const uint8_t* __restrict__ tu, TuSetDev s, int log2ctb, int32_t* status) {
    const int w4 = s.w / 4, h4 = s.h / 4;
    const int64_t total = s.tu_plane * s.nplanes;
    bool bad = false;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pl = i / s.tu_plane;
        const int u = (int)(i - pl * s.tu_plane), uy = u / w4, ux = u - uy * w4;
        bad |= !tu_unit_valid(tu + pl * s.tu_plane, w4, h4, ux, uy, log2ctb);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicMax(status, 2);
}

// ---------------------------------------------------------------------------
// Host side: every refusal before any HIP call.
// ---------------------------------------------------------------------------
static int rd_layout(const nh_plane_set* set, int ctb, int qp, int64_t lambda, TuSetDev& d, const char* who) {
    if (!set) {
        set_error(std::string(who) + ": null argument");
        return NH_EARG;
    }
    if (ctb != 16 && ctb != 32) {
        set_error(std::string(who) + ": ctb must be 16 or 32");
        return NH_EARG;
    }
    if (qp < 0 || qp > 51) {
        set_error(std::string(who) + ": qp must be in 0..51");
        return NH_EARG;
    }
    if (lambda < 0 || lambda > 2147483647ll) {
        set_error(std::string(who) + ": lambda must be in 0..2^31-1");
        return NH_EARG;
    }
    if ((set->width & 3) || (set->height & 3)) {
        set_error(std::string(who) + ": width and height must be multiples of 4");
        return NH_EARG;
    }
    if (set->width < 4 || set->height < 4 || set->width > 65532 || set->height > 65532 || set->pitch < set->width ||
        set->planes_per_group < 0 || set->num_groups < 0 || set->base < 0 || set->plane_stride < 0 || set->group_stride < 0) {
        set_error(std::string(who) + ": plane set must have sizes in 4..65532, pitch >= width, non-negative offsets and counts");
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
    if (np * d.rcols * d.rrows >= (1ll << 31) || np * d.tu_plane >= (1ll << 40)) {
        set_error(std::string(who) + ": too many planes (>= 2^31 regions)");
        return NH_EARG;
    }
    d.nplanes = (int32_t)np;
    d.aligned = !((set->base | set->plane_stride | set->group_stride | set->pitch) & 3);
    return NH_OK;
}

static int rd_launch(bool search, const int16_t* d_src, const nh_plane_set* set, int ctb, int is_luma, int qp,
                     int64_t lambda, int32_t* d_lvl, int16_t* d_recon, uint8_t* d_tu, uint8_t* d_pm, int64_t* d_stats,
                     void* d_work, void* stream, const char* who) {
    if (!d_src || !d_lvl || !d_recon || !d_tu || !d_pm || !d_stats || !set || (!search && !d_work)) {
        set_error(std::string(who) + ": null argument");
        return NH_EARG;
    }
    TuRdArgs a{};
    NH_TRY(rd_layout(set, ctb, qp, lambda, a.s, who));
    if (((uintptr_t)d_src & 1) || ((uintptr_t)d_lvl & 3) || ((uintptr_t)d_recon & 1) || ((uintptr_t)d_stats & 7) ||
        ((uintptr_t)d_work & 3)) {
        set_error(std::string(who) + ": buffers must be aligned to their element size");
        return NH_EARG;
    }
    if (!a.s.nplanes) return NH_OK;
    a.s.aligned = a.s.aligned && !((uintptr_t)d_src & 7) && !((uintptr_t)d_lvl & 15) && !((uintptr_t)d_recon & 7);
    a.src = d_src;
    a.lvl = d_lvl;
    a.rec = d_recon;
    a.tu = d_tu;
    a.pm = d_pm;
    a.stats = reinterpret_cast<unsigned long long*>(d_stats);
    a.work = static_cast<const int32_t*>(d_work);
    a.lam = lambda;
    a.log2ctb = ctb == 32 ? 5 : 4;
    a.is_luma = is_luma ? 1 : 0;
    const int per = qp / 6, rem = qp % 6;
    for (int l2 = 2; l2 <= 5; ++l2) {   // quant.py:41-79, intra rounding
        QuantParams& q = a.q[l2 - 2];
        q.shift = 14 + per + l2;
        q.mf = quant_scale(rem);
        q.off = (uint32_t)((1ull << q.shift) / 3);
    }
    a.dqs = dequant_scale(rem);
    a.dq_per = per;
    hipStream_t s = as_stream(stream);
    NH_HIP(hipMemsetAsync(d_stats, 0, 8ull * kRdStatsPerPlane * a.s.nplanes, s));
    const unsigned grid = (unsigned)((int64_t)a.s.nplanes * a.s.rcols * a.s.rrows);
    if (search) {
        k_tu_rd<true><<<grid, 256, 0, s>>>(a);
    } else {
        NH_HIP(hipMemsetAsync(d_work, 0, 4ull * kRdWorkWords, s));
        const int64_t units = a.s.tu_plane * a.s.nplanes;
        k_tu_rd_check<<<(unsigned)std::min<int64_t>(2048, (units + 255) / 256), 256, 0, s>>>(d_tu, a.s, a.log2ctb,
                                                                                            (int32_t*)d_work + 1);
        k_tu_rd<false><<<grid, 256, 0, s>>>(a);
    }
    NH_HIP(hipGetLastError());
    return NH_OK;
}

}  // namespace nh

using namespace nh;

extern "C" int nh_tu_rd_planes(const int16_t* d_src, const nh_plane_set* set, int ctb, int qp, int is_luma,
                               int64_t lambda, int32_t* d_lvl, int16_t* d_recon, uint8_t* d_tu, uint8_t* d_pm,
                               int64_t* d_stats, void* stream) {
    return rd_launch(true, d_src, set, ctb, is_luma, qp, lambda, d_lvl, d_recon, d_tu, d_pm, d_stats, nullptr, stream,
                     "nh_tu_rd_planes");
}

extern "C" int64_t nh_tu_encode_map_workspace_bytes(void) { return 4ll * kRdWorkWords; }

extern "C" int nh_tu_encode_map_planes(const int16_t* d_src, const uint8_t* d_tu, const nh_plane_set* set, int ctb,
                                       int qp, int is_luma, int64_t lambda, int32_t* d_lvl, int16_t* d_recon,
                                       uint8_t* d_pm, int64_t* d_stats, void* d_work, void* stream) {
    return rd_launch(false, d_src, set, ctb, is_luma, qp, lambda, d_lvl, d_recon, const_cast<uint8_t*>(d_tu), d_pm,
                     d_stats, d_work, stream, "nh_tu_encode_map_planes");
}
