// nh_rdo_n.hip -- config 3 at the other HEVC sizes: the 35-mode open-loop RDO
// per full NxN block for N = 4 (DST or DCT), 16 and 32.
//
// Per block: neighbours from the source plane with the BlockView rules
// (block.py:38-55; 128 outside the plane, numpy slice truncation of the 2N
// angular references at the right / bottom edge), planar / DC / 33 angular
// predictions (intra.py:46-62, :81-113, :116-207 with D5, D6, D8), and per mode
// the chain of k_tu_process (nh_intraloop.hip): residual -> forward transform ->
// quantize -> dequantize -> inverse transform -> reconstruct -> clip, cost =
// SSE(orig, recon) in 64 bits.  Lowest (sse << 6 | mode) wins.
//
// Work maps:
//   N = 4      a lane per (block, mode), the 4x4 in registers, 7 blocks x 35
//              modes per 256-thread workgroup (as k_intra_rdo8 does for 8x8);
//   N = 16, 32 N lanes per (block, mode) chain -- lane t does column t, then
//              row t, through an LDS tile of pitch N + 1 (as k_tu_process) --
//              7 chains per block, 5 rounds for the 35 modes, then chain 0 runs
//              the winning mode once more and stores its levels and recon.  A
//              workgroup is 224 lanes: one 32x32 block or two 16x16 blocks.
//              The block's samples and its 4N + 1 reference samples are staged
//              in LDS once for all 35 chains.  A chain lies inside one wave, so
//              the only workgroup barriers are the two after staging and the
//              one before the winner's round; between a chain's passes a
//              wave-level barrier orders the LDS accesses (a wave's LDS
//              instructions execute in program order).
// Blocks are independent (open loop): no cross-workgroup wait of any kind.
//
// Multiplies: the chain is k_tu_process's, whose 24-bit multiplies are exact for
// every int16 residual at every QP and size; tools/rdo_n_bounds.py enumerates the
// operand bounds for the transforms used here (tests/test_rdo_n_host.py).
//
// The CLOSED loop at the same sizes (second half of the
// file): the same chains, neighbours from the reconstruction, on the row
// wavefront of the N = 8 closed loop.  Its residual is int16 whatever the
// prediction, so the operand bounds above hold for it as they are.
//
// The closed loop's DECODER at the same sizes (the last
// kernel): stage P, one prediction per block on the same row wavefront, after
// stage R (nh_decode_n.hip) has put the residuals in place.
//
// Both loops with a RATE term: the kernels carry
// a compile-time RD flag.  RD = true: the key is J = D + lambda * R with R =
// count_nonzero(level) + 1 in place of the SSE, and (sum J, sum D, sum R) per
// plane are accumulated.  The RD entry points serve N = 8 from the N-lane chains
// as well.  RD = false is what the entry points without a rate term launch;
// every RD statement is under `if constexpr`.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <string>
#include "nh_common.hpp"
#include "nh_internal.hpp"
#include "nh_closed_ticket.hpp"
#include "nh_decode_n.hpp"

namespace nh {
namespace {

constexpr int kModesN = 35;
constexpr int kLaneSlots = 7;    // N = 4: blocks per workgroup
constexpr int kChains = 7;       // N = 16 / 32: chains per block

struct RdoNArgs {
    const int16_t* src;
    int32_t* lvl;
    int16_t* recon;
    uint8_t* modes;
    unsigned long long* sse;     // one word per plane, or null
    int32_t w, h, pitch;
    QuantParams qp;
    int32_t dq_scale, dq_per;
    int32_t vec_out;             // every row start of lvl / recon is 16-B aligned
    int64_t group_stride, plane_stride;
    int32_t ppg;
    // the RD form (§3.3b) only: J = D + lambda * R, three words per plane (sum J, sum D, sum R)
    unsigned long long lambda;
    unsigned long long* stats;
};
constexpr int kRdoStats = 3;

__device__ __forceinline__ int32_t w16(int32_t v) { return (int32_t)(int16_t)(uint16_t)(uint32_t)v; }

// INTRA_PRED_ANGLE[mode - 2] / INV_ANGLE[angle] for a per-lane mode without a
// memory table (the forms of nh_intraloop.hip's intra_angle_alu / inv_angle_alu)
__device__ __forceinline__ int angle_of(int mode) {
    constexpr uint64_t kMag = 0ull | (2ull << 6) | (5ull << 12) | (9ull << 18) | (13ull << 24) | (17ull << 30) |
                              (21ull << 36) | (26ull << 42) | (32ull << 48);
    const int d = mode < 18 ? 10 - mode : mode - 26;
    const int k = d < 0 ? -d : d;
    const int m = (int)((kMag >> (6 * k)) & 63);
    return d < 0 ? -m : m;
}
__device__ __forceinline__ int inv_angle_of(int angle) {
    constexpr uint64_t kLo = 4096ull | (1638ull << 13) | (910ull << 26) | (630ull << 39);
    constexpr uint64_t kHi = 482ull | (390ull << 13) | (315ull << 26) | (256ull << 39);
    const int a = -angle;
    const int k = a == 2 ? 0 : a == 5 ? 1 : a == 9 ? 2 : a == 13 ? 3 : a == 17 ? 4 : a == 21 ? 5 : a == 26 ? 6 : 7;
    const uint64_t t = k < 4 ? kLo : kHi;
    return -(int)((t >> (13 * (k & 3))) & 8191);
}

// One block's staged samples: orig, and [tl] + up to 2N top / left samples.
// ntA / nlA are the lengths of topA / leftA (N + 1 .. 2N + 1): an index past
// the end reads the last sample (intra.py:175-178, D6) -- the clamp, never a
// read beyond the plane rectangle.
template <int N>
struct RdoNBlock {
    int16_t orig[N * N];
    int16_t topA[2 * N + 2], leftA[2 * N + 2];
    int32_t ntA, nlA;
    int32_t dc;
    int32_t valid;
    unsigned long long best;
};

// Stage block (bx, by) with `nthr` cooperating threads (this one is `tid`).
template <int N>
__device__ __forceinline__ void stage_block(RdoNBlock<N>& B, const int16_t* __restrict__ src, int w, int h, int pitch,
                                            int bx, int by, int tid, int nthr) {
    const int x = bx * N, y = by * N;
    for (int e = tid; e < N * N; e += nthr)
        B.orig[e] = src[(int64_t)(y + e / N) * pitch + x + (e % N)];
    for (int e = tid; e < 4 * N; e += nthr) {
        const bool top = e < 2 * N;
        const int k = top ? e : e - 2 * N;
        // top row samples x .. x+2N-1 (block.py:38-43) / left column y .. y+2N-1 (block.py:45-50)
        const bool in = top ? (y > 0 && x + k < w) : (x > 0 && y + k < h);
        int16_t v = 128;
        if (in) v = top ? src[(int64_t)(y - 1) * pitch + x + k] : src[(int64_t)(y + k) * pitch + x - 1];
        (top ? B.topA : B.leftA)[1 + k] = v;
    }
    if (tid == 0) {
        const int16_t tl = (x > 0 && y > 0) ? src[(int64_t)(y - 1) * pitch + x - 1] : (int16_t)128;
        B.topA[0] = tl;
        B.leftA[0] = tl;
        B.ntA = 1 + (y == 0 ? 2 * N : min(2 * N, w - x));
        B.nlA = 1 + (x == 0 ? 2 * N : min(2 * N, h - y));
    }
}
template <int N>
__device__ __forceinline__ int32_t block_dc(const RdoNBlock<N>& B) {   // intra.py:61, floor division (D7)
    int32_t s = 0;
    for (int k = 1; k <= N; ++k) s += B.topA[k] + B.leftA[k];
    return (s + N) >> (Log2<N>::v + 1);
}
template <int N>
__device__ __forceinline__ int32_t planar_at(const RdoNBlock<N>& B, int y, int x) {   // intra.py:107-111
    return ((N - 1 - x) * B.leftA[1 + y] + (x + 1) * B.topA[N] + (N - 1 - y) * B.topA[1 + x] + (y + 1) * B.leftA[N] + N) >>
           (Log2<N>::v + 1);
}

// _build_ref_array (intra.py:159-188): logical element i in [-N, 2N] of the
// reference array of one angular mode.
struct AngCtx {
    const int16_t *pri, *sec;
    int np, ns, angle, inv, next;
};
template <int N, class B_>
__device__ __forceinline__ AngCtx ang_ctx(const B_& B, int mode) {
    AngCtx a;
    const bool vert = mode >= 18;
    a.pri = vert ? B.topA : B.leftA;
    a.sec = vert ? B.leftA : B.topA;
    a.np = vert ? B.ntA : B.nlA;
    a.ns = vert ? B.nlA : B.ntA;
    a.angle = angle_of(mode);
    a.inv = a.angle < 0 ? inv_angle_of(a.angle) : 0;
    a.next = (N * a.angle) >> 5;
    return a;
}
__device__ __forceinline__ int32_t ref_at(const AngCtx& a, int i) {
    if (i >= 0) return a.pri[i < a.np ? i : a.np - 1];
    if (a.angle < 0 && i >= a.next) {
        const int proj = ((i + 1) * a.inv + 128) >> 8;   // (i + 1): D5
        if (proj < a.ns) return a.sec[proj];
    }
    return 0;
}
// _project_sample_at (intra.py:191-207) on r0 = ref[idx], r1 = ref[idx + 1]: int16 arithmetic (D8)
__device__ __forceinline__ int32_t interp(int32_t r0, int32_t r1, int f) {
    const int32_t v = w16((32 - f) * r0 + f * r1 + 16) >> 5;
    return f ? v : r0;
}

__device__ __forceinline__ int32_t clip8(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// levels / recon rows of one thread: 16-B pieces when aligned, elements otherwise
template <int N>
__device__ __forceinline__ void store_lvl_row(int32_t* row, const int32_t (&l)[N], bool vec) {
    if (vec) {
#pragma unroll
        for (int j = 0; j < N; j += 4) *(int4*)(row + j) = make_int4(l[j], l[j + 1], l[j + 2], l[j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = l[j];
    }
}
template <int N>
__device__ __forceinline__ void store_rec_row(int16_t* row, const uint32_t (&p)[N / 2], bool vec) {
    if (vec) {
        if constexpr (N == 4) {
            *(uint2*)row = make_uint2(p[0], p[1]);       // x0 is a multiple of 4: 8-B aligned
        } else {
#pragma unroll
            for (int j = 0; j < N / 2; j += 4) *(uint4*)(row + 2 * j) = make_uint4(p[j], p[j + 1], p[j + 2], p[j + 3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = (int16_t)(p[j / 2] >> (16 * (j & 1)));
    }
}

__device__ __forceinline__ void plane_offsets(RdoNArgs& a, int nblk) {
    const int pz = (int)blockIdx.y, gz = pz / a.ppg;
    const int64_t poff = (int64_t)gz * a.group_stride + (int64_t)(pz - gz * a.ppg) * a.plane_stride;
    a.src += poff;
    a.lvl += poff;
    a.recon += poff;
    a.modes += (int64_t)pz * nblk;
    if (a.sse) a.sse += pz;
}

// One 4x4 (block, mode) chain of one lane, the block in registers: prediction from the staged
// neighbours, residual -> transform -> quantize -> dequantize -> inverse -> reconstruct -> clip.
// Lv: the levels, Rp: the recon as int16 pairs, both row-major; returns the SSE.
template <bool DST>
__device__ __forceinline__ unsigned long long lane_chain4(const RdoNBlock<4>& L, int mode, const ChainQ& cq,
                                                          int32_t (&Lv)[4][4], uint32_t (&Rp)[4][2]) {
    constexpr int N = 4, S = Log2<N>::v + 5;
    int32_t P[N][N];
    if (mode >= 2) {
        const AngCtx ac = ang_ctx<N>(L, mode);
        const bool vert = mode >= 18;
        int32_t Q[N][N];
#pragma unroll
        for (int scan = 0; scan < N; ++scan) {
            const int proj = (scan + 1) * ac.angle, f = proj & 31;
#pragma unroll
            for (int base = 0; base < N; ++base) {
                const int i = base + 1 + (proj >> 5);
                Q[scan][base] = interp(ref_at(ac, i), ref_at(ac, i + 1), f);
            }
        }
        // pred[y = scan][x = base] for vertical modes, transposed otherwise (intra.py:145-154)
#pragma unroll
        for (int y = 0; y < N; ++y)
#pragma unroll
            for (int x = 0; x < N; ++x) P[y][x] = vert ? Q[y][x] : Q[x][y];
    } else {
#pragma unroll
        for (int y = 0; y < N; ++y)
#pragma unroll
            for (int x = 0; x < N; ++x) P[y][x] = mode == 0 ? planar_at<N>(L, y, x) : L.dc;
    }
    uint32_t X[N][N];
#pragma unroll
    for (int y = 0; y < N; ++y)
#pragma unroll
        for (int x = 0; x < N; ++x) X[y][x] = (uint32_t)w16((int32_t)L.orig[y * N + x] - P[y][x]);   // residual_block
#pragma unroll
    for (int j = 0; j < N; ++j) {   // forward pass 1: columns
        uint32_t x[N], y[N];
#pragma unroll
        for (int k = 0; k < N; ++k) x[k] = X[k][j];
        fwd1d<N, DST, Mul24>(x, y);
#pragma unroll
        for (int i = 0; i < N; ++i) X[i][j] = (uint32_t)rshift_round<S>(y[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {   // forward pass 2: rows, quantize, dequantize
        uint32_t y[N];
        fwd1d<N, DST, Mul24>(X[i], y);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            Lv[i][j] = quant_s(rshift_round<S>(y[j]), cq.qs, cq.h_v, cq.hneg_v);
            X[i][j] = (uint32_t)dequant_s(Lv[i][j], cq);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {   // inverse pass 1: columns
        uint32_t yv[N], x[N];
#pragma unroll
        for (int k = 0; k < N; ++k) yv[k] = X[k][j];
        inv1d<N, DST, Mul24>(yv, x);
#pragma unroll
        for (int i = 0; i < N; ++i) X[i][j] = (uint32_t)rshift_round<S>(x[i]);
    }
    unsigned long long sse = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {   // inverse pass 2: rows, reconstruct, clip, SSE
        uint32_t x[N];
        inv1d<N, DST, Mul24>(X[i], x);
        int32_t rc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            rc[j] = clip8(w16(P[i][j] + w16(rshift_round<S>(x[j]))));
            const int32_t d = w16((int32_t)L.orig[i * N + j] - rc[j]);
            sse += (unsigned long long)(uint32_t)(d * d);
        }
#pragma unroll
        for (int j = 0; j < N; j += 2) Rp[i][j / 2] = (uint32_t)rc[j] | ((uint32_t)rc[j + 1] << 16);
    }
    return sse;
}

// ---------------------------------------------------------------------------
// N = 4: lane = (block slot, mode)
// ---------------------------------------------------------------------------
// nonzero levels of a 4x4 held in registers (the RD form's rate, §3.3b)
__device__ __forceinline__ int32_t nnz4(const int32_t (&Lv)[4][4]) {
    int32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) n += Lv[i][j] != 0;
    return n;
}

// RD: the key is J = D + lambda * (nnz + 1) instead of the SSE, and the workgroup adds (sum J, sum D,
// sum R) of its blocks to the plane's three stats words (§3.3b).
template <bool DST, bool RD>
__device__ __forceinline__ void rdo_n_lane(RdoNArgs a) {
    constexpr int N = 4;
    __shared__ RdoNBlock<N> B[kLaneSlots];
    __shared__ unsigned long long wg_sse;
    __shared__ unsigned long long wg_dr[RD ? 2 : 1];   // RD: sum D, sum R of the workgroup
    const int bw = a.w / N, nblk = bw * (a.h / N);
    plane_offsets(a, nblk);
    const int t = threadIdx.x;
    const int slot = t / kModesN, mode = t - slot * kModesN;
    const int b0 = (int)blockIdx.x * kLaneSlots;
    {   // 32 threads stage a block
        const int sb = t / 32, st = t % 32;
        if (sb < kLaneSlots) {
            const int b = b0 + sb;
            if (b < nblk) stage_block<N>(B[sb], a.src, a.w, a.h, a.pitch, b % bw, b / bw, st, 32);
            if (st == 0) {
                B[sb].valid = b < nblk;
                B[sb].best = ULLONG_MAX;
            }
        }
        if (t == 0) wg_sse = 0;
        if constexpr (RD) {
            if (t < 2) wg_dr[t] = 0;
        }
    }
    __syncthreads();
    if (t < kLaneSlots && B[t].valid) B[t].dc = block_dc<N>(B[t]);
    __syncthreads();
    const bool active = slot < kLaneSlots && B[slot < kLaneSlots ? slot : 0].valid;
    const RdoNBlock<N>& L = B[slot < kLaneSlots ? slot : 0];
    const ChainQ cq = make_chainq(a.qp, a.dq_scale, a.dq_per);
    int32_t Lv[N][N];
    uint32_t Rp[N][N / 2];
    unsigned long long key = ULLONG_MAX, dist = 0, rate = 0;
    if (active) {
        dist = lane_chain4<DST>(L, mode, cq, Lv, Rp);
        if constexpr (RD) {
            rate = (unsigned long long)(nnz4(Lv) + 1);
            key = ((dist + a.lambda * rate) << 6) | (unsigned long long)mode;
        } else {
            key = (dist << 6) | (unsigned long long)mode;
        }
        atomicMin(&B[slot].best, key);
    }
    __syncthreads();
    if (active && key == L.best) {
        const int b = b0 + slot;
        const int by = b / bw, bx = b - by * bw;
        a.modes[b] = (uint8_t)mode;
        atomicAdd(&wg_sse, key >> 6);
        if constexpr (RD) {
            atomicAdd(&wg_dr[0], dist);
            atomicAdd(&wg_dr[1], rate);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int64_t o = (int64_t)(by * N + i) * a.pitch + bx * N;
            store_lvl_row<N>(a.lvl + o, Lv[i], a.vec_out);
            store_rec_row<N>(a.recon + o, Rp[i], a.vec_out);
        }
    }
    __syncthreads();
    if constexpr (RD) {
        if (t < kRdoStats) atomicAdd(a.stats + kRdoStats * (int64_t)blockIdx.y + t, t == 0 ? wg_sse : wg_dr[t - 1]);
    } else {
        if (a.sse && t == 0) atomicAdd(a.sse, wg_sse);   // once per workgroup
    }
}

// ---------------------------------------------------------------------------
// N = 16 / 32: N lanes per (block, mode) chain
// ---------------------------------------------------------------------------
// Between an LDS write and another lane's read inside one chain: the chain's
// lanes are in one wave, whose LDS instructions execute in program order, so
// only the compiler has to keep the order.
__device__ __forceinline__ void chain_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One (block, mode) chain on the N lanes of a chain: lane t does column t, then row t, through
// the chain's LDS tile (pitch N + 1); rf: the chain's 3N + 2 angular reference samples.  Returns
// the SSE of row t; rcp: row t of the recon as int16 pairs.  lvl_row (the winner's round): where
// lane t stores row t of the levels, or null.  RD: *nnz receives the nonzero levels of row t.
template <int N, bool RD = false>
__device__ __forceinline__ unsigned long long tile_chain(const RdoNBlock<N>& L, int mode, int t, int32_t (*tile)[N + 1],
                                                         int16_t* rf, const ChainQ& cq, int32_t* lvl_row, bool vec,
                                                         uint32_t (&rcp)[N / 2], int32_t* nnz = nullptr) {
    constexpr int S = Log2<N>::v + 5;
    int angle = 0;
    const bool vert = mode >= 18;
    if (mode >= 2) {
        const AngCtx ac = ang_ctx<N>(L, mode);
        angle = ac.angle;
        for (int i = t; i < 3 * N + 2; i += N) rf[i] = i <= 3 * N ? (int16_t)ref_at(ac, i - N) : (int16_t)0;
    }
    chain_sync();
    auto pred_at = [&](int y, int x) -> int32_t {
        if (mode == 0) return planar_at<N>(L, y, x);
        if (mode == 1) return L.dc;
        const int base = vert ? x : y, scan = vert ? y : x;
        const int proj = (scan + 1) * angle;
        const int16_t* rp = rf + N + base + 1 + (proj >> 5);
        return interp(rp[0], rp[1], proj & 31);
    };
    uint32_t v[N], q[N];
    // forward pass 1 on column t of the residual
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (uint32_t)w16((int32_t)L.orig[k * N + t] - pred_at(k, t));
    fwd1d<N, false, Mul24>(v, q);
#pragma unroll
    for (int i = 0; i < N; ++i) tile[i][t] = rshift_round<S>(q[i]);
    chain_sync();
    // forward pass 2 on row t, quantize, dequantize (row t is this lane's own)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[t][k];
    fwd1d<N, false, Mul24>(v, q);
    {
        int32_t l[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            l[j] = quant_s(rshift_round<S>(q[j]), cq.qs, cq.h_v, cq.hneg_v);
            tile[t][j] = dequant_s(l[j], cq);
        }
        if (lvl_row) store_lvl_row<N>(lvl_row, l, vec);
        if constexpr (RD) {
            int32_t c = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) c += l[j] != 0;
            *nnz = c;
        }
    }
    chain_sync();
    // inverse pass 1 on column t (this lane's own column)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[k][t];
    inv1d<N, false, Mul24>(v, q);
#pragma unroll
    for (int i = 0; i < N; ++i) tile[i][t] = rshift_round<S>(q[i]);
    chain_sync();
    // inverse pass 2 on row t, reconstruct, clip, SSE
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (uint32_t)tile[t][k];
    inv1d<N, false, Mul24>(v, q);
    unsigned long long sse = 0;
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        int32_t rc2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            rc2[u] = clip8(w16(pred_at(t, j + u) + w16(rshift_round<S>(q[j + u]))));
            const int32_t d = w16((int32_t)L.orig[t * N + j + u] - rc2[u]);
            sse += (unsigned long long)(uint32_t)(d * d);
        }
        rcp[j / 2] = (uint32_t)rc2[0] | ((uint32_t)rc2[1] << 16);
    }
    return sse;
}

// RD (§3.3b): a chain lane contributes sse_row + lambda * nnz_row, so the N-lane sum is D + lambda * nnz;
// lane 0 of the chain adds lambda once.  The winner's round follows the loop: chain 0 of every block
// sums the nonzero levels of its rerun (R = nnz + 1, J = best >> 6, D = J - lambda * R), and the
// workgroup adds one (sum J, sum D, sum R) to the plane's stats words.
template <int N, bool RD>
__device__ __forceinline__ void rdo_n_tile(RdoNArgs a) {
    constexpr int BPW = 32 / N;                 // blocks per workgroup
    constexpr int NC = kChains * BPW;           // chains per workgroup
    constexpr int NT = NC * N;                  // 224 threads
    constexpr int P = N + 1;
    __shared__ RdoNBlock<N> B[BPW];
    __shared__ int32_t tile[NC][N][P];
    __shared__ int16_t refs[NC][3 * N + 2];
    __shared__ unsigned long long wg_st[RD ? kRdoStats : 1];
    const int bw = a.w / N, nblk = bw * (a.h / N);
    plane_offsets(a, nblk);
    const int tid = threadIdx.x;
    const int ci = tid / N, t = tid % N;
    const int blk = ci / kChains, c = ci - blk * kChains;
    if constexpr (RD) {
        if (tid < kRdoStats) wg_st[tid] = 0;    // ordered by the barriers of the staging below
    }
    const int b0 = (int)blockIdx.x * BPW;
    for (int k = 0; k < BPW; ++k) {
        const int b = b0 + k;
        if (b < nblk) stage_block<N>(B[k], a.src, a.w, a.h, a.pitch, b % bw, b / bw, tid, NT);
        if (tid == 0) {
            B[k].valid = b < nblk;
            B[k].best = ULLONG_MAX;
        }
    }
    __syncthreads();
    if (tid < BPW && B[tid].valid) B[tid].dc = block_dc<N>(B[tid]);
    __syncthreads();
    const RdoNBlock<N>& L = B[blk];
    const bool on = L.valid != 0;
    const ChainQ cq = make_chainq(a.qp, a.dq_scale, a.dq_per);
    const int b = b0 + blk;
    const int y0 = (b / bw) * N, x0 = (b % bw) * N;
    int16_t* rf = refs[ci];

    for (int r = 0; r <= kModesN / kChains; ++r) {
        const bool emit = r == kModesN / kChains;      // the winner's round
        if (emit) {
            __syncthreads();                           // every chain's key is in L.best
            if constexpr (RD) break;                   // the RD winner's round is below the loop
            if (tid == 0 && a.sse) {
                unsigned long long s = 0;
                for (int k = 0; k < BPW; ++k)
                    if (B[k].valid) s += B[k].best >> 6;
                atomicAdd(a.sse, s);                   // once per workgroup
            }
            if (!on || c != 0) return;
        }
        if (!on) continue;
        const int mode = emit ? (int)(L.best & 63) : r * kChains + c;
        uint32_t rcp[N / 2];
        int32_t nnz = 0;
        unsigned long long sse = tile_chain<N, RD>(L, mode, t, tile[ci], rf, cq,
                                                   emit ? a.lvl + (int64_t)(y0 + t) * a.pitch + x0 : nullptr, a.vec_out,
                                                   rcp, &nnz);
        if constexpr (RD) sse += a.lambda * (unsigned long long)nnz;
        if (emit) {
            store_rec_row<N>(a.recon + (int64_t)(y0 + t) * a.pitch + x0, rcp, a.vec_out);
            if (t == 0) a.modes[b] = (uint8_t)mode;
            return;
        }
        // the chain's SSE: sum over its N lanes (an aligned group of N lanes of the wave)
#pragma unroll
        for (int m = N / 2; m >= 1; m >>= 1) sse += __shfl_xor(sse, m);
        if constexpr (RD) sse += a.lambda;             // R = nnz + 1
        if (t == 0) atomicMin(&B[blk].best, (sse << 6) | (unsigned long long)mode);
        chain_sync();   // refs / tile are rewritten by the next round
    }
    if constexpr (RD) {
        if (on && c == 0) {
            const unsigned long long best = L.best;
            const int mode = (int)(best & 63);
            uint32_t rcp[N / 2];
            int32_t nnz = 0;
            tile_chain<N, true>(L, mode, t, tile[ci], rf, cq, a.lvl + (int64_t)(y0 + t) * a.pitch + x0, a.vec_out, rcp,
                                &nnz);
            store_rec_row<N>(a.recon + (int64_t)(y0 + t) * a.pitch + x0, rcp, a.vec_out);
#pragma unroll
            for (int m = N / 2; m >= 1; m >>= 1) nnz += __shfl_xor(nnz, m);
            if (t == 0) {
                a.modes[b] = (uint8_t)mode;
                const unsigned long long J = best >> 6, R = (unsigned long long)(nnz + 1);
                atomicAdd(&wg_st[0], J);
                atomicAdd(&wg_st[1], J - a.lambda * R);
                atomicAdd(&wg_st[2], R);
            }
        }
        __syncthreads();
        // once per workgroup
        if (tid < kRdoStats) atomicAdd(a.stats + kRdoStats * (int64_t)blockIdx.y + tid, wg_st[tid]);
    }
}

// The RD form at N = 32 needs 174 VGPRs where the plain form needs 144: held to the plain form's three
// waves per SIMD (168 VGPRs, no scratch).  A bound of 1 is the default: the plain forms compile as before.
template <int N, bool DST, bool RD = false>
__global__ void __launch_bounds__(N == 4 ? 256 : 224) __attribute__((amdgpu_waves_per_eu(RD && N == 32 ? 3 : 1)))
k_intra_rdo_n(RdoNArgs a) {
    if constexpr (N == 4) rdo_n_lane<DST, RD>(a); else rdo_n_tile<N, RD>(a);
}

void split_qp(int qp, int log2n, QuantParams* q, int* per, int* rem) {
    *per = qp / 6;
    *rem = qp % 6;
    q->shift = 14 + *per + log2n;
    q->mf = quant_scale(*rem);
    q->off = (uint32_t)((1ull << q->shift) / 3);   // intra rounding (quant.py:66-69)
}

// ===========================================================================
// CLOSED loop at N = 4, 16, 32: blocks in raster order,
// every neighbour from the reconstruction built so far.  The schedule is
// k_intra_rdo8_closed_tag's (nh_intraloop.hip, §4.3a): a worker per block row,
// rows claimed by an atomic ticket in closed_ticket's order 1, so a worker only
// waits on a row claimed before its own; block bx of row r needs blocks
// <= bx + 1 of row r - 1.  A block's bottom row is published as N / 2 tagged
// 64-bit words ((row + 1) << 32 | int16 pair), one system-scope relaxed store
// each; the row below polls the N words of its top and top-right blocks until
// their tags name the row above.  Words past the last full block are never
// written and read as 0 without a wait.  Row r + 1 overwrites block bx's words
// only after it has read them for its blocks bx - 1 and bx; the top-left sample
// is carried from the previous block's top read, and the previous block's
// right column (LDS) is the left reference.  A wait longer than
// kClosedNSpinLimit polls, or one that finds the status word set, sets status 1
// at work[1] and the worker leaves; every other waiter then leaves too.
// ===========================================================================
struct ClosedNSet {
    int64_t base, plane_stride, group_stride;
    int32_t w, h, pitch, ppg;
    int32_t bw, bh, row0, plane0;   // full blocks per row / column; first global row / plane of this set
    int64_t mode0;                  // first mode-map entry of this set
    int64_t line0;                  // first line word of this set
    int32_t lw;                     // line words per plane
    int32_t np;                     // planes in this set
    int32_t vec_out;                // every row start of lvl / recon is 16-B aligned
};
struct ClosedNArgs {
    const int16_t* src;
    int32_t* lvl;
    int16_t* rec;
    uint8_t* modes;
    unsigned long long* sse;        // per plane (accumulated)
    int32_t* work;                  // [0] ticket, [1] status, from word kClosedNLines0 the 64-bit line words
    ClosedNSet set[NH_MAX_PLANE_SETS];
    int32_t nsets, total_rows;
    int32_t order, max_bh;          // closed_ticket: order 1 (row-major across planes), largest bh
    int64_t lines_total;
    QuantParams qp;
    int32_t dq_scale, dq_per;
    unsigned long long lambda;      // the RD form (§3.7b) only; sse then holds three words per plane
};
constexpr int kClosedNLines0 = 2;           // int32 words before the line words (8-B aligned)
constexpr int kClosedNSpinLimit = 1 << 20;  // as kSpinLimit of the N = 8 kernel: ~1 s of polling

// the coherent accesses of nh_intraloop.hip's closed loop, restated
__device__ __forceinline__ int cn_ld_sys(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t cn_ld_sys64(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void cn_st_sys64(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The calling wave (all 64 lanes) waits for the N line words x0/2 .. x0/2 + N - 1 of the row
// above block row `by`: lane k < N polls word k until its tag is `by`; val: the word's int16
// pair (0 for a word past the last full block, which is not waited for).  False: the wait ran
// out or another worker has set the status word -- status 1 is set and the caller leaves.
template <int N>
__device__ __forceinline__ bool poll_top(const uint64_t* line, int x0, int full_words, int by, int lane, int32_t* work,
                                         uint32_t& val) {
    const int wi = x0 / 2 + lane;
    const bool need = lane < N && wi < full_words;
    val = 0;
    int spins = 0;
    for (;;) {
        bool ok = true;
        if (need) {
            const uint64_t v = cn_ld_sys64(line + wi);
            ok = (int)(v >> 32) == by;
            val = (uint32_t)v;
        }
        if (__builtin_amdgcn_read_exec() == __ballot(ok)) return true;   // every needed word is there
        __builtin_amdgcn_s_sleep(1);
        ++spins;
        if (spins > kClosedNSpinLimit || ((spins & 1023) == 0 && cn_ld_sys(&work[1]))) {
            if (lane == 0) atomicMax(&work[1], 1);
            return false;
        }
    }
}

struct ClosedNRow {
    const int16_t* src;
    int32_t* lvl;
    int16_t* rec;
    uint64_t* line;
    uint8_t* modes;     // the row's first mode-map entry
};
__device__ __forceinline__ ClosedNRow closed_row(const ClosedNArgs& a, const ClosedNSet& S, int pl, int by) {
    const int g = pl / S.ppg, c = pl - g * S.ppg;
    const int64_t off = S.base + (int64_t)g * S.group_stride + (int64_t)c * S.plane_stride;
    ClosedNRow r;
    r.src = a.src + off;
    r.lvl = a.lvl + off;
    r.rec = a.rec + off;
    r.line = reinterpret_cast<uint64_t*>(a.work + kClosedNLines0) + S.line0 + (int64_t)pl * S.lw;
    r.modes = a.modes + S.mode0 + ((int64_t)pl * S.bh + by) * S.bw;
    return r;
}

// The neighbours of block (bx, by) into B: thread k of `first` .. first + 3N.  topw: the N line
// words of the row above (int16 pairs), leftcol: the previous block's right column, tl: the
// carried top-left sample.
template <int N>
__device__ __forceinline__ void closed_stage_refs(RdoNBlock<N>& B, int k, const uint32_t* topw, const int16_t* leftcol,
                                                  int x0, int y0, int w, int16_t tl) {
    if (k < 0) return;
    if (k < 2 * N) {
        int16_t v = 128;
        if (y0 > 0 && x0 + k < w) v = (int16_t)(topw[k >> 1] >> ((k & 1) * 16));
        B.topA[1 + k] = v;
    } else if (k < 3 * N) {
        B.leftA[1 + k - 2 * N] = x0 == 0 ? (int16_t)128 : leftcol[k - 2 * N];
    } else if (k == 3 * N) {
        const int16_t c = (y0 == 0 || x0 == 0) ? (int16_t)128 : tl;
        B.topA[0] = c;
        B.leftA[0] = c;
        B.ntA = 1 + (y0 == 0 ? 2 * N : min(2 * N, w - x0));   // numpy's slice ends at the plane's right edge
        B.nlA = 1 + N;                                        // the bottom-left is not coded yet
        B.best = ULLONG_MAX;
    }
}

// N = 4: one wave per block row, a lane per mode, the block in registers (lane_chain4).
// RD (§3.7b): the key is J = D + lambda * (nnz + 1), and the row adds (sum J, sum D, sum R) to its plane's
// three words at a.sse.
template <bool DST, bool RD = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RD ? 4 : 1)))   // RD: 128 VGPRs as the plain form
k_intra_rdo_closed_lane(ClosedNArgs a) {
    constexpr int N = 4;
    __shared__ RdoNBlock<N> B;
    __shared__ uint32_t topw[N];
    __shared__ int16_t leftcol[N];
    __shared__ int row_s, stall_s;
    const int lane = threadIdx.x;
    const ChainQ cq = make_chainq(a.qp, a.dq_scale, a.dq_per);
    for (;;) {
        if (lane == 0) {
            row_s = atomicAdd(&a.work[0], 1);
            stall_s = 0;
        }
        __syncthreads();
        const int row = row_s;
        if (row >= a.total_rows) break;
        int si, pl, by;
        closed_ticket(a, row, si, pl, by);
        const ClosedNSet& S = a.set[si];
        const ClosedNRow R = closed_row(a, S, pl, by);
        const int y0 = by * N, full_words = S.bw * (N / 2);
        int16_t tl_next = 128;
        unsigned long long row_sse = 0, row_d = 0, row_r = 0;   // row_d, row_r: RD only
        for (int bx = 0; bx < S.bw; ++bx) {
            const int x0 = bx * N;
            int16_t ov = 0;
            if (lane < N * N) ov = R.src[(int64_t)(y0 + lane / N) * S.pitch + x0 + (lane % N)];
            if (by > 0) {
                uint32_t val;
                if (!poll_top<N>(R.line, x0, full_words, by, lane, a.work, val)) stall_s = 1;
                if (lane < N) topw[lane] = val;
            }
            __syncthreads();
            if (stall_s) break;
            if (lane < N * N) B.orig[lane] = ov;
            closed_stage_refs<N>(B, lane - N * N, topw, leftcol, x0, y0, S.w, tl_next);
            __syncthreads();
            if (lane == 0) B.dc = block_dc<N>(B);
            tl_next = B.topA[N];
            __syncthreads();
            int32_t Lv[N][N];
            uint32_t Rp[N][N / 2];
            unsigned long long key = ULLONG_MAX, dist = 0, rate = 0;
            if (lane < kModesN) {
                dist = lane_chain4<DST>(B, lane, cq, Lv, Rp);
                if constexpr (RD) {
                    rate = (unsigned long long)(nnz4(Lv) + 1);
                    key = ((dist + a.lambda * rate) << 6) | (unsigned long long)lane;
                } else {
                    key = (dist << 6) | (unsigned long long)lane;
                }
            }
            unsigned long long best = key;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long o = __shfl_xor(best, m);
                best = o < best ? o : best;
            }
            if (key == best) {   // one lane: the mode is part of the key
                // publish the bottom row first (the next row polls these words)
                const uint64_t tag = (uint64_t)(uint32_t)(by + 1) << 32;
#pragma unroll
                for (int q = 0; q < N / 2; ++q) cn_st_sys64(R.line + x0 / 2 + q, tag | Rp[N - 1][q]);
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    leftcol[i] = (int16_t)(Rp[i][N / 2 - 1] >> 16);
                    const int64_t o = (int64_t)(y0 + i) * S.pitch + x0;
                    store_lvl_row<N>(R.lvl + o, Lv[i], S.vec_out);
                    store_rec_row<N>(R.rec + o, Rp[i], S.vec_out);
                }
                R.modes[bx] = (uint8_t)lane;
                row_sse += best >> 6;
                if constexpr (RD) {
                    row_d += dist;
                    row_r += rate;
                }
            }
            __syncthreads();   // leftcol is there; B is free for the next block
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) row_sse += __shfl_xor(row_sse, m);
        if constexpr (RD) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                row_d += __shfl_xor(row_d, m);
                row_r += __shfl_xor(row_r, m);
            }
            if (lane < kRdoStats && row_r)
                atomicAdd(&a.sse[kRdoStats * (int64_t)(S.plane0 + pl) + lane],
                          lane == 0 ? row_sse : lane == 1 ? row_d : row_r);
        } else {
            if (lane == 0 && row_sse) atomicAdd(&a.sse[S.plane0 + pl], row_sse);
        }
        const int stalled = stall_s;
        __syncthreads();       // before lane 0 resets stall_s for the next row
        if (stalled) break;
    }
}

// N = 16 / 32: one 224-lane workgroup per block row, N lanes per (block, mode) chain
// (tile_chain): 14 chains over 3 rounds at N = 16, 7 chains over 5 rounds at N = 32, then chain 0
// runs the winner once more and stores its levels and recon.  Wave 0 polls; the words and the
// stall flag reach the others through LDS and a workgroup barrier.  Every thread passes the same
// barriers: the stall exit is taken by all of them after the same barrier.
// RD (§3.7b): the chains' keys as in rdo_n_tile's RD form; chain 0 sums the nonzero levels of the winner's
// rerun, and thread 0 adds the row's (sum J, sum D, sum R) to its plane's three words at a.sse.
template <int N, bool RD = false>
__global__ void __launch_bounds__(224) __attribute__((amdgpu_waves_per_eu(RD && N == 16 ? 4 : 1)))   // <= 128 VGPRs
k_intra_rdo_closed_tile(ClosedNArgs a) {
    constexpr int NT = 224, NC = NT / N, ROUNDS = (kModesN + NC - 1) / NC, P = N + 1;
    constexpr int OV = (N * N + NT - 1) / NT;   // source samples per thread
    static_assert(3 * N + 1 <= NT && N <= 64, "neighbour staging and the poll need that many threads");
    __shared__ RdoNBlock<N> B;
    __shared__ int32_t tile[NC][N][P];
    __shared__ int16_t refs[NC][3 * N + 2];
    __shared__ uint32_t topw[N];
    __shared__ int16_t leftcol[N];
    __shared__ int row_s, stall_s;
    const int tid = threadIdx.x;
    const int ci = tid / N, t = tid % N;
    const ChainQ cq = make_chainq(a.qp, a.dq_scale, a.dq_per);
    for (;;) {
        if (tid == 0) {
            row_s = atomicAdd(&a.work[0], 1);
            stall_s = 0;
        }
        __syncthreads();
        const int row = row_s;
        if (row >= a.total_rows) break;
        int si, pl, by;
        closed_ticket(a, row, si, pl, by);
        const ClosedNSet& S = a.set[si];
        const ClosedNRow R = closed_row(a, S, pl, by);
        const int y0 = by * N, full_words = S.bw * (N / 2);
        int16_t tl_next = 128;              // thread 3N's
        unsigned long long row_sse = 0;     // thread 0's
        unsigned long long row_d = 0, row_r = 0;   // thread 0's, RD only
        for (int bx = 0; bx < S.bw; ++bx) {
            const int x0 = bx * N;
            int16_t ov[OV];
#pragma unroll
            for (int k = 0; k < OV; ++k) {
                const int e = tid + k * NT;
                ov[k] = e < N * N ? R.src[(int64_t)(y0 + e / N) * S.pitch + x0 + (e % N)] : (int16_t)0;
            }
            if (by > 0 && tid < 64) {       // wave 0
                uint32_t val;
                if (!poll_top<N>(R.line, x0, full_words, by, tid, a.work, val)) stall_s = 1;
                if (tid < N) topw[tid] = val;
            }
            __syncthreads();
            if (stall_s) break;             // the same value in every thread: written before the barrier only
#pragma unroll
            for (int k = 0; k < OV; ++k) {
                const int e = tid + k * NT;
                if (e < N * N) B.orig[e] = ov[k];
            }
            closed_stage_refs<N>(B, tid, topw, leftcol, x0, y0, S.w, tl_next);
            __syncthreads();
            if (tid == 0) B.dc = block_dc<N>(B);
            if (tid == 3 * N) tl_next = B.topA[N];
            __syncthreads();
            for (int r = 0; r < ROUNDS; ++r) {
                const int mode = r * NC + ci;
                if (mode < kModesN) {
                    uint32_t rcp[N / 2];
                    int32_t nnz = 0;
                    unsigned long long sse =
                        tile_chain<N, RD>(B, mode, t, tile[ci], refs[ci], cq, nullptr, false, rcp, &nnz);
                    if constexpr (RD) sse += a.lambda * (unsigned long long)nnz;
                    // the chain's SSE: sum over its N lanes (an aligned group of N lanes of the wave)
#pragma unroll
                    for (int m = N / 2; m >= 1; m >>= 1) sse += __shfl_xor(sse, m);
                    if constexpr (RD) sse += a.lambda;   // R = nnz + 1
                    if (t == 0) atomicMin(&B.best, (sse << 6) | (unsigned long long)mode);
                    chain_sync();           // refs / tile are rewritten by the next round
                }
            }
            __syncthreads();                // every chain's key is in B.best
            if (ci == 0) {
                const unsigned long long best = B.best;
                const int mode = (int)(best & 63);
                const int64_t o = (int64_t)(y0 + t) * S.pitch + x0;
                uint32_t rcp[N / 2];
                int32_t nnz = 0;
                tile_chain<N, RD>(B, mode, t, tile[0], refs[0], cq, R.lvl + o, S.vec_out != 0, rcp, &nnz);
                if (t == N - 1) {           // publish the bottom row first (the next row polls these words)
                    const uint64_t tag = (uint64_t)(uint32_t)(by + 1) << 32;
#pragma unroll
                    for (int q = 0; q < N / 2; ++q) cn_st_sys64(R.line + x0 / 2 + q, tag | rcp[q]);
                }
                leftcol[t] = (int16_t)(rcp[N / 2 - 1] >> 16);
                store_rec_row<N>(R.rec + o, rcp, S.vec_out != 0);
                if constexpr (RD) {
#pragma unroll
                    for (int m = N / 2; m >= 1; m >>= 1) nnz += __shfl_xor(nnz, m);
                }
                if (t == 0) {
                    R.modes[bx] = (uint8_t)mode;
                    row_sse += best >> 6;
                    if constexpr (RD) {
                        const unsigned long long r = (unsigned long long)(nnz + 1);
                        row_d += (best >> 6) - a.lambda * r;
                        row_r += r;
                    }
                }
            }
            __syncthreads();                // leftcol is there; B, topw are free for the next block
        }
        if constexpr (RD) {
            if (tid == 0 && row_r) {
                unsigned long long* st = &a.sse[kRdoStats * (int64_t)(S.plane0 + pl)];
                atomicAdd(st, row_sse);
                atomicAdd(st + 1, row_d);
                atomicAdd(st + 2, row_r);
            }
        } else {
            if (tid == 0 && row_sse) atomicAdd(&a.sse[S.plane0 + pl], row_sse);
        }
        const int stalled = stall_s;
        __syncthreads();                    // before thread 0 resets stall_s for the next row
        if (stalled) break;
    }
}

// Samples outside full NxN blocks read as 0 (Plane.zeros) by the closed loop.
__global__ void __launch_bounds__(256) k_zero_partial_n(int16_t* rec, ClosedNSet S, int n) {
    const int p = blockIdx.y;
    const int g = p / S.ppg, c = p - g * S.ppg;
    int16_t* r = rec + S.base + (int64_t)g * S.group_stride + (int64_t)c * S.plane_stride;
    const int fw = S.bw * n, fh = S.bh * n;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < (int64_t)S.w * S.h; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / S.w), x = (int)(i - (int64_t)y * S.w);
        if (x >= fw || y >= fh) r[(int64_t)y * S.pitch + x] = 0;
    }
}

// The refusals the two RD entry points add to check_rdo_n_args' (nh_decode_n.hip); `who` names the caller.
int check_rd_args(const char* who, const nh_plane_set* sets, int nsets, int block_size, int use_dst, int qp,
                  int64_t lambda, const void* d_stats) {
    NH_TRY(check_rdo_n_args(who, sets, nsets, block_size, use_dst, qp));
    if (lambda < 0 || lambda > 0x7fffffffll) {
        set_error(std::string(who) + ": lambda outside 0..2^31-1");
        return NH_EARG;
    }
    if ((uintptr_t)d_stats & 7) {
        set_error(std::string(who) + ": d_stats must be 8-byte aligned");
        return NH_EARG;
    }
    return NH_OK;
}

int64_t planes_of(const nh_plane_set* sets, int nsets) {
    int64_t n = 0;
    for (int k = 0; k < nsets; ++k) n += (int64_t)sets[k].planes_per_group * sets[k].num_groups;
    return n;
}

// Rows, planes, mode-map and line-word offsets of the closed loop at block size n.  The sets have
// passed check_rdo_n_args' plane-set test.  NH_EARG, with `who` in the error text: a plane wider or
// higher than 65535 samples, or 2^30 block rows and more.
int closed_n_layout(const char* who, const nh_plane_set* sets, int nsets, int n, ClosedNArgs& a) {
    const auto refuse = [who] {
        set_error(std::string(who) + ": bad plane set (sizes <= 65535, < 2^30 block rows)");
        return NH_EARG;
    };
    int64_t rows = 0, planes = 0, modes = 0, lines = 0;
    a.max_bh = 0;
    for (int k = 0; k < nsets; ++k) {
        const nh_plane_set& p = sets[k];
        if (p.width > 65535 || p.height > 65535) return refuse();
        ClosedNSet& S = a.set[k];
        S.base = p.base;
        S.plane_stride = p.plane_stride;
        S.group_stride = p.group_stride;
        S.w = p.width;
        S.h = p.height;
        S.pitch = p.pitch;
        S.ppg = p.planes_per_group;
        S.bw = p.width / n;
        S.bh = S.bw ? p.height / n : 0;   // a plane narrower than a block has no row to code
        S.row0 = (int32_t)rows;
        S.plane0 = (int32_t)planes;
        S.mode0 = modes;
        S.lw = (p.width + 1) / 2 + n;     // int16 pairs + the top-right read past the last block
        S.line0 = lines;
        const int64_t np = (int64_t)p.planes_per_group * p.num_groups;
        S.np = (int32_t)np;
        S.vec_out = !(p.pitch & 7) && !((p.base | p.plane_stride | p.group_stride) & 7);
        if (S.bh > a.max_bh) a.max_bh = S.bh;
        rows += np * S.bh;
        planes += np;
        modes += np * (p.width / n) * (p.height / n);
        lines += np * S.lw;
        if (rows >= (1ll << 30)) return refuse();
    }
    a.nsets = nsets;
    a.total_rows = (int32_t)rows;
    a.order = 1;
    a.lines_total = lines;
    return NH_OK;
}

template <class K>
int launch_closed_n(K kern, int threads, const ClosedNArgs& a, hipStream_t s) {
    // persistent workers: one per row, capped at what can be resident (a worker only ever waits on
    // a row claimed before its own, so fewer workers than rows is always safe)
    int cus = 0, per_cu = 0;
    NH_TRY(device_cus(&cus));
    NH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0));
    const int64_t cap = (int64_t)std::max(1, per_cu) * cus;
    kern<<<(unsigned)(a.total_rows < cap ? a.total_rows : cap), threads, 0, s>>>(a);
    NH_HIP(hipGetLastError());
    return NH_OK;
}

// ===========================================================================
// Closed-loop DECODER at N = 4, 16, 32: mode map +
// levels -> the reconstruction of nh_intra_rdo_planes_closed_n.  Stage R
// (k_dequant_inv_n, nh_decode_n.hip, earlier on the stream) has put every
// block's residual into rec; this kernel is the dependent part, stage P.  The
// schedule is the encoder's above: ClosedNArgs / closed_row / poll_top /
// launch_closed_n and, on the host, closed_n_begin as they are, rows claimed by ticket in
// closed_ticket's order 1, tagged 64-bit line words, the bottom row published
// before the block's recon stores, the top-left sample and the left column
// carried along the row, the bounded poll, work[1] honoured by every waiter.
// One wave per block row at every N -- no workgroup barrier anywhere: lane t
// holds S = max(1, N * N / 64) neighbouring samples of one block row (1 / 4 / 16
// at N = 4 / 16 / 32; lanes 16 .. 63 idle at N = 4).  Per block: poll the N words
// of the top and top-right blocks, ONE prediction (the mode is uniform over the
// block, so planar / DC / angular are scalar branches) from the staged
// references in LDS, + residual (int16 wrap), clip, publish, store over the
// residual the samples came from.  The next block's residual and mode are
// fetched under the current wait.  Neighbours are read from line words, LDS and
// registers only, never from rec.  Every neighbour is a clipped 8-bit sample or
// 128, so the int16 arithmetic of intra.py never wraps in the predictors.
// ===========================================================================
// Pre-pass, the test of k_dec_check_modes (nh_intraloop.hip): a mode above 34 sets status 2.
__global__ void __launch_bounds__(256) k_dec_check_modes_n(const uint8_t* __restrict__ modes, int64_t n,
                                                           int32_t* status) {
    bool bad = false;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bad |= modes[i] >= kModesN;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicMax(status, 2);
}

// The staged references of one block, as ang_ctx reads them: [tl] + 2N top samples, [tl] + N left samples.
struct DecNRefs {
    const int16_t *topA, *leftA;
    int32_t ntA, nlA;
};

template <int N>
__global__ void __launch_bounds__(64) k_intra_dec_closed_n(ClosedNArgs a) {
    constexpr int S = N * N >= 64 ? N * N / 64 : 1;   // samples per lane
    constexpr int LPR = N / S;                        // lanes per block row
    constexpr int LG = Log2<N>::v;
    if (cn_ld_sys(&a.work[1])) return;   // bad mode map: no row is claimed, nothing waits
    __shared__ int16_t topA[2 * N + 2], leftA[N + 2], rf[3 * N + 2];
    const int lane = threadIdx.x;
    const bool act = lane < N * LPR;
    const int i = act ? lane / LPR : 0, j0 = act ? (lane % LPR) * S : 0;   // this lane: row i, columns j0 .. j0 + S - 1
    for (;;) {
        int t = 0;
        if (lane == 0) t = atomicAdd(&a.work[0], 1);
        const int row = __builtin_amdgcn_readfirstlane(t);
        if (row >= a.total_rows) break;
        int si, pl, by;
        closed_ticket(a, row, si, pl, by);
        const ClosedNSet& Z = a.set[si];
        const ClosedNRow R = closed_row(a, Z, pl, by);
        const int y0 = by * N, full_words = Z.bw * (N / 2);
        const bool vec = Z.vec_out != 0;
        int16_t* p = R.rec + (int64_t)(y0 + i) * Z.pitch + j0;   // this lane's samples of block 0 of the row
        const uint64_t tag = (uint64_t)(uint32_t)(by + 1) << 32;
        auto load_res = [&](int x0, int32_t (&r)[S]) {
            if (!act) {
#pragma unroll
                for (int k = 0; k < S; ++k) r[k] = 0;
            } else if (S >= 4 && vec) {
#pragma unroll
                for (int k = 0; k < S; k += 4) {
                    const uint2 q = *reinterpret_cast<const uint2*>(p + x0 + k);   // 8-B aligned: j0 + k is a multiple of 4
                    r[k] = (int16_t)q.x;
                    r[k + 1] = (int32_t)q.x >> 16;
                    r[k + 2] = (int16_t)q.y;
                    r[k + 3] = (int32_t)q.y >> 16;
                }
            } else {
#pragma unroll
                for (int k = 0; k < S; ++k) r[k] = p[x0 + k];
            }
        };
        int tl = 128;            // top[N - 1] of the previous block: the next block's top-left (its line word is overwritten)
        int32_t res_n[S];
        int m_n = 0;
        load_res(0, res_n);      // bw >= 1: a plane narrower than a block has no row
        m_n = R.modes[0];
        if (lane < N) leftA[1 + lane] = 128;   // no block to the left
        bool stall = false;
        for (int bx = 0; bx < Z.bw; ++bx) {
            const int x0 = bx * N;
            int32_t res[S];
#pragma unroll
            for (int k = 0; k < S; ++k) res[k] = res_n[k];
            const int m = __builtin_amdgcn_readfirstlane(m_n);
            if (bx + 1 < Z.bw) {   // next block's residual and mode, under this block's wait
                load_res(x0 + N, res_n);
                m_n = R.modes[bx + 1];
            }
            uint32_t val = 0;
            if (by > 0) {
                const bool ok = poll_top<N>(R.line, x0, full_words, by, lane, a.work, val);
                if (__ballot(!ok)) {
                    stall = true;
                    break;
                }
            }
            // stage the references (closed_stage_refs' rules): 128 above the plane and right of it
            if (lane < N) {
                const int k = 2 * lane;
                topA[1 + k] = (y0 > 0 && x0 + k < Z.w) ? (int16_t)val : (int16_t)128;
                topA[2 + k] = (y0 > 0 && x0 + k + 1 < Z.w) ? (int16_t)(val >> 16) : (int16_t)128;
            }
            const int tlc = (by == 0 || bx == 0) ? 128 : tl;
            if (lane == 0) {
                topA[0] = (int16_t)tlc;
                leftA[0] = (int16_t)tlc;
            }
            chain_sync();
            tl = topA[N];
            DecNRefs B;
            B.topA = topA;
            B.leftA = leftA;
            B.ntA = 1 + (by == 0 ? 2 * N : min(2 * N, Z.w - x0));   // numpy's slice ends at the plane's right edge
            B.nlA = 1 + N;                                          // the bottom-left is not coded yet
            int32_t v[S];
            if (m == 0) {          // planar, tr = top[N - 1], bl = left[N - 1] (intra.py:81-113)
                const int lv = leftA[1 + i], tr = topA[N], bl = leftA[N];
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const int x = j0 + k;
                    v[k] = ((N - 1 - x) * lv + (x + 1) * tr + (N - 1 - i) * topA[1 + x] + (i + 1) * bl + N) >> (LG + 1);
                }
            } else if (m == 1) {   // DC (intra.py:46-62), floor division
                int s = lane < N ? topA[1 + lane] + leftA[1 + lane] : 0;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                const int dc = (s + N) >> (LG + 1);
#pragma unroll
                for (int k = 0; k < S; ++k) v[k] = dc;
            } else {               // angular (intra.py:116-207): the reference array once per block, in LDS
                const AngCtx ac = ang_ctx<N>(B, m);
                for (int e = lane; e < 3 * N + 2; e += 64) rf[e] = e <= 3 * N ? (int16_t)ref_at(ac, e - N) : (int16_t)0;
                chain_sync();
                const bool vert = m >= 18;
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const int x = j0 + k;
                    const int base = vert ? x : i, scan = vert ? i : x;
                    const int proj = (scan + 1) * ac.angle;
                    const int16_t* rp = rf + N + base + 1 + (proj >> 5);
                    v[k] = interp(rp[0], rp[1], proj & 31);
                }
            }
            // reconstruct_block (int16 wrap) + clip_to_pixel_range(., 8)
#pragma unroll
            for (int k = 0; k < S; ++k) v[k] = clip8(w16(v[k] + res[k]));
            // publish the bottom row first (the next row polls these words)
            if constexpr (S == 1) {
                const int hi = __shfl(v[0], (lane + 1) & 63, 64);
                if (act && i == N - 1 && !(j0 & 1))
                    cn_st_sys64(R.line + (x0 + j0) / 2, tag | (uint32_t)v[0] | ((uint32_t)hi << 16));
            } else {
                if (i == N - 1) {
#pragma unroll
                    for (int k = 0; k < S; k += 2)
                        cn_st_sys64(R.line + (x0 + j0 + k) / 2, tag | (uint32_t)v[k] | ((uint32_t)v[k + 1] << 16));
                }
            }
            chain_sync();          // every lane has read leftA / topA / rf of this block
            if (act && j0 + S == N) leftA[1 + i] = (int16_t)v[S - 1];   // the next block's left column
            if (act) {
                if (S >= 4 && vec) {
#pragma unroll
                    for (int k = 0; k < S; k += 4)
                        *reinterpret_cast<uint2*>(p + x0 + k) = make_uint2((uint32_t)v[k] | ((uint32_t)v[k + 1] << 16),
                                                                           (uint32_t)v[k + 2] | ((uint32_t)v[k + 3] << 16));
                } else {
#pragma unroll
                    for (int k = 0; k < S; ++k) p[x0 + k] = (int16_t)v[k];
                }
            }
        }
        if (stall) break;
        chain_sync();              // the next row's first writes to leftA come after this row's last reads
    }
}

// ===========================================================================
// Host side: one launch path per form -- open loop, closed-loop encoder -- and
// one start for everything on the row wavefront, the decoder included.  RD picks
// the kernels with the rate term, which serve N = 8 on
// the N-lane chains too (4 blocks per workgroup in the open loop, 28 chains over
// 2 rounds in the closed loop); without it N = 8 never gets here.
// ===========================================================================
template <class A>
void set_qp(A& a, int qp, int N) {
    int per, rem;
    split_qp(qp, log2_of(N), &a.qp, &per, &rem);
    a.dq_scale = dequant_scale(rem);
    a.dq_per = per;
}

// The open loop, a launch per set that holds a block.  d_acc: the per-plane sums the kernels add to -- RD:
// three words per plane (sum J, sum D, sum R); otherwise one (the SSE), or null for none.
template <bool RD>
int launch_rdo_n(const int16_t* d_src, const nh_plane_set* sets, int nsets, int N, int use_dst, int qp, int64_t lambda,
                 uint8_t* d_modes, int32_t* d_lvl, int16_t* d_recon, int64_t* d_acc, hipStream_t s) {
    RdoNArgs a{};
    set_qp(a, qp, N);
    a.lambda = (unsigned long long)lambda;
    const int bpw = N == 4 ? kLaneSlots : 32 / N, threads = N == 4 ? 256 : 224;   // blocks per workgroup
    int64_t moff = 0, soff = 0;
    for (int k = 0; k < nsets; ++k) {
        const nh_plane_set& S = sets[k];
        const int64_t planes = (int64_t)S.planes_per_group * S.num_groups;
        const int nblk = (S.width / N) * (S.height / N);
        if (nblk && planes) {
            a.src = d_src + S.base;
            a.lvl = d_lvl + S.base;
            a.recon = d_recon + S.base;
            a.modes = d_modes + moff;
            if constexpr (RD) a.stats = (unsigned long long*)(d_acc + kRdoStats * soff);
            else a.sse = d_acc ? (unsigned long long*)(d_acc + soff) : nullptr;
            a.w = S.width;
            a.h = S.height;
            a.pitch = S.pitch;
            a.vec_out = !(S.pitch & 7) && !((S.base | S.plane_stride | S.group_stride) & 7) &&
                        !((uintptr_t)d_lvl & 15) && !((uintptr_t)d_recon & 15);
            a.group_stride = S.group_stride;
            a.plane_stride = S.plane_stride;
            a.ppg = S.planes_per_group;
            const dim3 grid((unsigned)((nblk + bpw - 1) / bpw), (unsigned)planes);
            if (N == 4 && use_dst) k_intra_rdo_n<4, true, RD><<<grid, threads, 0, s>>>(a);
            else if (N == 4) k_intra_rdo_n<4, false, RD><<<grid, threads, 0, s>>>(a);
            else if (N == 16) k_intra_rdo_n<16, false, RD><<<grid, threads, 0, s>>>(a);
            else if (N == 32) k_intra_rdo_n<32, false, RD><<<grid, threads, 0, s>>>(a);
            else if constexpr (RD) k_intra_rdo_n<8, false, true><<<grid, threads, 0, s>>>(a);
            NH_HIP(hipGetLastError());
        }
        moff += planes * nblk;
        soff += planes;
    }
    return NH_OK;
}

int64_t closed_n_work_bytes(const ClosedNArgs& a) { return 4ll * kClosedNLines0 + 8ll * a.lines_total; }

// The *_workspace_bytes entry points: -1 with the refusal in nh_last_error.  at8: the 8x8 function that
// N = 8 forwards to, or null where N = 8 runs on the line words of this file (the RD form).
int64_t closed_n_workspace_bytes(const char* who, const nh_plane_set* sets, int nsets, int block_size,
                                 int64_t (*at8)(const nh_plane_set*, int)) {
    if (!sets) {
        set_error(std::string(who) + ": null argument");
        return -1;
    }
    if (check_rdo_n_args(who, sets, nsets, block_size, 0, 0)) return -1;
    if (block_size == 8 && at8) return at8(sets, nsets);
    ClosedNArgs a;
    if (closed_n_layout(who, sets, nsets, block_size, a)) return -1;
    return closed_n_work_bytes(a);
}

// How every call on the row wavefront starts; a.rec, a.work (and a.sse) are the caller's already.  First
// the refusals, before any device call: the layout's, the workspace's and, elem_ok false, the decoder's own.
// Then the workspace zeroed (ticket, status, line tags), zero_stats: the kRdoStats words per plane at a.sse
// zeroed, vec_out dropped unless the caller's buffers are 16-B aligned (vec_ok), and every sample outside
// full blocks set to 0.
int closed_n_begin(const char* who, const nh_plane_set* sets, int nsets, int N, ClosedNArgs& a, hipStream_t s,
                   bool vec_ok, bool zero_stats = false, bool elem_ok = true) {
    NH_TRY(closed_n_layout(who, sets, nsets, N, a));
    if ((uintptr_t)a.work & 7) {
        set_error(std::string(who) + ": workspace must be 8-byte aligned");
        return NH_EARG;
    }
    if (!elem_ok) {
        set_error(std::string(who) + ": buffers must be aligned to their element size");
        return NH_EARG;
    }
    NH_HIP(hipMemsetAsync(a.work, 0, (size_t)closed_n_work_bytes(a), s));
    const int64_t planes = planes_of(sets, nsets);
    if (zero_stats && planes) NH_HIP(hipMemsetAsync(a.sse, 0, 8ull * kRdoStats * (uint64_t)planes, s));
    for (int k = 0; k < nsets; ++k) {
        a.set[k].vec_out = a.set[k].vec_out && vec_ok;
        if (a.set[k].np > 0 && (int64_t)a.set[k].w * a.set[k].h > 0)
            k_zero_partial_n<<<dim3(64, (unsigned)a.set[k].np), 256, 0, s>>>(a.rec, a.set[k], N);
    }
    NH_HIP(hipGetLastError());
    return NH_OK;
}

// The closed-loop encoder.  d_acc: the per-plane sums as launch_rdo_n's; RD zeroes them, without it the
// kernels add to what the caller put there.
template <bool RD>
int launch_rdo_closed_n(const char* who, const int16_t* d_src, const nh_plane_set* sets, int nsets, int N, int use_dst,
                        int qp, int64_t lambda, uint8_t* d_modes, int32_t* d_lvl, int16_t* d_recon, int64_t* d_acc,
                        void* d_work, hipStream_t s) {
    ClosedNArgs a{};
    a.src = d_src;
    a.lvl = d_lvl;
    a.rec = d_recon;
    a.modes = d_modes;
    a.sse = (unsigned long long*)d_acc;
    a.work = (int32_t*)d_work;
    NH_TRY(closed_n_begin(who, sets, nsets, N, a, s, !((uintptr_t)d_lvl & 15) && !((uintptr_t)d_recon & 15), RD));
    set_qp(a, qp, N);
    a.lambda = (unsigned long long)lambda;
    if (a.total_rows <= 0) return NH_OK;
    if (N == 4 && use_dst) return launch_closed_n(k_intra_rdo_closed_lane<true, RD>, 64, a, s);
    if (N == 4) return launch_closed_n(k_intra_rdo_closed_lane<false, RD>, 64, a, s);
    if (N == 16) return launch_closed_n(k_intra_rdo_closed_tile<16, RD>, 224, a, s);
    if (N == 32) return launch_closed_n(k_intra_rdo_closed_tile<32, RD>, 224, a, s);
    if constexpr (RD) return launch_closed_n(k_intra_rdo_closed_tile<8, true>, 224, a, s);
    return NH_OK;
}

}  // namespace
}  // namespace nh

using namespace nh;

extern "C" int nh_intra_rdo_planes_n(const int16_t* d_src, const nh_plane_set* sets, int nsets, int block_size,
                                     int use_dst, int qp, uint8_t* d_modes, int32_t* d_lvl, int16_t* d_recon,
                                     int64_t* d_sse, void* stream) {
    if (!d_src || !sets || !d_modes || !d_lvl || !d_recon) {
        set_error("nh_intra_rdo_planes_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rdo_n_args("nh_intra_rdo_planes_n", sets, nsets, block_size, use_dst, qp));
    if (block_size == 8) return nh_intra_rdo_planes(d_src, sets, nsets, qp, d_modes, d_lvl, d_recon, d_sse, stream);
    return launch_rdo_n<false>(d_src, sets, nsets, block_size, use_dst, qp, 0, d_modes, d_lvl, d_recon, d_sse,
                               as_stream(stream));
}

extern "C" int nh_intra_rdo_rd_planes_n(const int16_t* d_src, const nh_plane_set* sets, int nsets, int block_size,
                                        int use_dst, int qp, int64_t lambda, uint8_t* d_modes, int32_t* d_lvl,
                                        int16_t* d_recon, int64_t* d_stats, void* stream) {
    if (!d_src || !sets || !d_modes || !d_lvl || !d_recon || !d_stats) {
        set_error("nh_intra_rdo_rd_planes_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rd_args("nh_intra_rdo_rd_planes_n", sets, nsets, block_size, use_dst, qp, lambda, d_stats));
    const int64_t planes = planes_of(sets, nsets);
    if (!planes) return NH_OK;   // nothing to code, no stats word to zero
    const hipStream_t s = as_stream(stream);
    NH_HIP(hipMemsetAsync(d_stats, 0, 8ull * kRdoStats * (uint64_t)planes, s));
    return launch_rdo_n<true>(d_src, sets, nsets, block_size, use_dst, qp, lambda, d_modes, d_lvl, d_recon, d_stats, s);
}

extern "C" int64_t nh_intra_rdo_closed_n_workspace_bytes(const nh_plane_set* sets, int nsets, int block_size) {
    return closed_n_workspace_bytes("nh_intra_rdo_closed_n_workspace_bytes", sets, nsets, block_size,
                                    nh_intra_rdo_closed_workspace_bytes);
}

extern "C" int64_t nh_intra_rdo_rd_closed_n_workspace_bytes(const nh_plane_set* sets, int nsets, int block_size) {
    return closed_n_workspace_bytes("nh_intra_rdo_rd_closed_n_workspace_bytes", sets, nsets, block_size, nullptr);
}

extern "C" int64_t nh_intra_decode_closed_n_workspace_bytes(const nh_plane_set* sets, int nsets, int block_size) {
    return closed_n_workspace_bytes("nh_intra_decode_closed_n_workspace_bytes", sets, nsets, block_size,
                                    nh_intra_decode_closed_workspace_bytes);
}

extern "C" int nh_intra_rdo_planes_closed_n(const int16_t* d_src, const nh_plane_set* sets, int nsets, int block_size,
                                            int use_dst, int qp, uint8_t* d_modes, int32_t* d_lvl, int16_t* d_recon,
                                            int64_t* d_sse, void* d_work, void* stream) {
    if (!d_src || !sets || !d_modes || !d_lvl || !d_recon || !d_sse || !d_work) {
        set_error("nh_intra_rdo_planes_closed_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rdo_n_args("nh_intra_rdo_planes_closed_n", sets, nsets, block_size, use_dst, qp));
    if (block_size == 8)
        return nh_intra_rdo_planes_closed(d_src, sets, nsets, qp, d_modes, d_lvl, d_recon, d_sse, d_work, stream);
    return launch_rdo_closed_n<false>("nh_intra_rdo_planes_closed_n", d_src, sets, nsets, block_size, use_dst, qp, 0,
                                      d_modes, d_lvl, d_recon, d_sse, d_work, as_stream(stream));
}

extern "C" int nh_intra_rdo_rd_planes_closed_n(const int16_t* d_src, const nh_plane_set* sets, int nsets,
                                               int block_size, int use_dst, int qp, int64_t lambda, uint8_t* d_modes,
                                               int32_t* d_lvl, int16_t* d_recon, int64_t* d_stats, void* d_work,
                                               void* stream) {
    if (!d_src || !sets || !d_modes || !d_lvl || !d_recon || !d_stats || !d_work) {
        set_error("nh_intra_rdo_rd_planes_closed_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rd_args("nh_intra_rdo_rd_planes_closed_n", sets, nsets, block_size, use_dst, qp, lambda, d_stats));
    return launch_rdo_closed_n<true>("nh_intra_rdo_rd_planes_closed_n", d_src, sets, nsets, block_size, use_dst, qp,
                                     lambda, d_modes, d_lvl, d_recon, d_stats, d_work, as_stream(stream));
}

extern "C" int nh_intra_decode_planes_closed_n(const uint8_t* d_modes, const int32_t* d_lvl, const nh_plane_set* sets,
                                               int nsets, int block_size, int use_dst, int qp, int16_t* d_recon,
                                               void* d_work, void* stream) {
    if (!d_modes || !d_lvl || !sets || !d_recon || !d_work) {
        set_error("nh_intra_decode_planes_closed_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rdo_n_args("nh_intra_decode_planes_closed_n", sets, nsets, block_size, use_dst, qp, false));
    if (block_size == 8) return nh_intra_decode_planes_closed(d_modes, d_lvl, sets, nsets, qp, d_recon, d_work, stream);
    const int N = block_size;
    ClosedNArgs a{};
    a.lvl = const_cast<int32_t*>(d_lvl);     // read only, by stage R (the encoder's argument block)
    a.rec = d_recon;
    a.modes = const_cast<uint8_t*>(d_modes);   // read only
    a.work = (int32_t*)d_work;
    const hipStream_t s = as_stream(stream);
    NH_TRY(closed_n_begin("nh_intra_decode_planes_closed_n", sets, nsets, N, a, s, !((uintptr_t)d_recon & 15), false,
                          !((uintptr_t)d_lvl & 3) && !((uintptr_t)d_recon & 1)));
    // stage R: every block's residual into d_recon (the wavefront reads neighbours only from line words, LDS
    // and registers, so a block's residual is read from, and its recon written to, the same place)
    NH_TRY(nh_dequant_inv_planes_n(d_lvl, 4, d_recon, sets, nsets, N, use_dst, qp, stream));
    const ClosedNSet& last = a.set[nsets - 1];
    const int64_t modes_total = last.mode0 + (int64_t)last.np * (last.w / N) * (last.h / N);
    if (modes_total > 0)
        k_dec_check_modes_n<<<(unsigned)std::min<int64_t>(1024, (modes_total + 255) / 256), 256, 0, s>>>(
            d_modes, modes_total, (int32_t*)d_work + 1);
    NH_HIP(hipGetLastError());
    if (a.total_rows > 0) {
        if (N == 4) NH_TRY(launch_closed_n(k_intra_dec_closed_n<4>, 64, a, s));
        else if (N == 16) NH_TRY(launch_closed_n(k_intra_dec_closed_n<16>, 64, a, s));
        else NH_TRY(launch_closed_n(k_intra_dec_closed_n<32>, 64, a, s));
    }
    return NH_OK;
}

