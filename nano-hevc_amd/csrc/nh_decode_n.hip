// nh_decode_n.hip -- stage R of the closed-loop decoder at N = 4 (DST or DCT), 16
// and 32.  Per full NxN block of int16 / int32 level
// planes
//   res = inverse_transform(dequantize_block(level, qp), use_dst).astype(np.int16)
// (quant.py:82-123, transform.py:199-238), written at the block's raster
// position; samples outside full blocks are left untouched.  The arithmetic is
// k_dequant_inv_tu's (nh_decode_tu.hip): ring arithmetic mod 2^32 throughout
// (64-bit dequantiser product and rounding shift, wrapping 32-bit products and
// sums in both passes, the low 16 bits at the end), so it is exact for EVERY
// level value of the input dtype; the matrix form of transform.py with the
// basis in LDS; both sums stop at the block's last nonzero level row / column.
// That kernel is driven by a TU map and needs widths that are multiples of 4;
// this one has one N for the call, takes any width, height, pitch and base,
// and covers every plane of every set in one launch: a 256-thread workgroup per
// 32x32 region of a plane's full-block area, a thread owns 4 neighbouring
// samples of one row (N is a multiple of 4: they lie in one block).  Blocks
// are independent: no wait of any kind.
#include <hip/hip_runtime.h>
#include <string>
#include "nh_common.hpp"
#include "nh_internal.hpp"
#include "nh_decode_n.hpp"

namespace nh {

namespace {

typedef short v4s __attribute__((ext_vector_type(4)));
typedef int v4w __attribute__((ext_vector_type(4)));

// The 32-point basis as bytes (|DCT32| <= 90), built at compile time and copied to LDS.
struct alignas(16) DeqNBasis32 {   // read as 32-bit words
    int8_t c[32][32];
};
constexpr DeqNBasis32 make_deqn_basis32() {
    DeqNBasis32 b{};
    for (int k = 0; k < 32; ++k)
        for (int n = 0; n < 32; ++n) b.c[k][n] = (int8_t)dct32(k, n);
    return b;
}
__constant__ DeqNBasis32 c_deqn_basis32 = make_deqn_basis32();

struct DeqNSet {
    int64_t base, plane_stride, group_stride;
    int32_t pitch, ppg;
    int32_t fw, fh;          // the full-block area: (w / N) * N by (h / N) * N samples
    int32_t rcols, rrows;    // 32x32 regions over it
    uint32_t wg_start;       // first workgroup of this set; 0xffffffff: no such set
};
struct DeqNArgs {
    const void* lvl;
    int16_t* res;
    DeqNSet set[NH_MAX_PLANE_SETS];
    int32_t log2n, dst;      // log2 N; 1: the 4x4 DST-VII
    int32_t scale, per;      // DEQUANT_SCALE[qp % 6], qp / 6
};

// LB: bytes per level (2 / 4).  ALIGNED: the 4 samples of a thread in one access (base, pitch and
// strides multiples of 8 elements, both buffers 16-B aligned); otherwise one element per access.
template <int LB, bool ALIGNED>
__global__ void __launch_bounds__(256) k_dequant_inv_n(DeqNArgs a) {
    __shared__ int32_t A[32][33], B[32][33];
    __shared__ int32_t T32[32][33];   // T32[k][n] = DCT32[k][n]; DCT_N[k][n] = T32[k * 32 / N][n]
    __shared__ int32_t D4[4][4];
    __shared__ int rext[64], cext[64];   // per block (slot of its top-left 4x4 unit): rows / columns up to the last nonzero level
    const int t = threadIdx.x;
    int si = 0;
#pragma unroll
    for (int k = 1; k < NH_MAX_PLANE_SETS; ++k)
        if (blockIdx.x >= a.set[k].wg_start) si = k;   // absent sets: 0xffffffff, empty sets: the next set's start
    const DeqNSet& s = a.set[si];
    const uint32_t local = blockIdx.x - s.wg_start;
    const uint32_t rpp = (uint32_t)s.rcols * (uint32_t)s.rrows;
    const int pl = local / rpp, r = local - pl * rpp;
    const int ry = r / s.rcols, rx = r - ry * s.rcols;
    {   // 4 basis bytes per thread
        const uint32_t q = reinterpret_cast<const uint32_t*>(&c_deqn_basis32.c[0][0])[t];
#pragma unroll
        for (int i = 0; i < 4; ++i) T32[t >> 3][(t & 7) * 4 + i] = (int32_t)(int8_t)(q >> (8 * i));
    }
    if (t < 16) D4[t >> 2][t & 3] = dst4c(t >> 2, t & 3);
    if (t < 64) {
        rext[t] = 0;
        cext[t] = 0;
    }
    // this thread: row lr of the region, columns lc .. lc + 3
    const int lr = t >> 3, lc = (t & 7) * 4;
    const int x = rx * 32 + lc, y = ry * 32 + lr;
    const bool on = x < s.fw && y < s.fh;   // fw is a multiple of 4: all four samples or none
    const int g = pl / s.ppg, c = pl - g * s.ppg;
    const int64_t off = s.base + (int64_t)g * s.group_stride + (int64_t)c * s.plane_stride + (int64_t)y * s.pitch + x;
    int32_t l[4] = {0, 0, 0, 0};
    if (on) {
        if constexpr (LB == 4) {
            const int32_t* p = static_cast<const int32_t*>(a.lvl) + off;
            if constexpr (ALIGNED) {
                const v4w q = *reinterpret_cast<const v4w*>(p);
                l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) l[i] = p[i];
            }
        } else {
            const int16_t* p = static_cast<const int16_t*>(a.lvl) + off;
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
    for (int i = 0; i < 4; ++i) A[lr][lc + i] = l[i] ? dequant_i32(l[i], a.scale, a.per) : 0;   // quant.py:112-123; 0 -> 0
    __syncthreads();
    const int v = a.log2n, n = 1 << v, step = 32 >> v;
    const int ty = lr & ~(n - 1), tx = lc & ~(n - 1);   // the block's origin in the region
    const int li = lr - ty, lj = lc - tx;
    // A zero level dequantises to 0 and a zero coefficient adds nothing to either pass, so both
    // sums stop at the block's last nonzero row / column: the same ring arithmetic minus zero terms
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
    const bool dst = a.dst != 0;
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
        int16_t* q = a.res + off;
        if constexpr (ALIGNED) {
            *reinterpret_cast<v4s*>(q) = v4s{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = o[i];
        }
    }
}

}  // namespace

int check_rdo_n_args(const char* who, const nh_plane_set* sets, int nsets, int block_size, int use_dst, int qp,
                     bool check_qp) {
    const std::string w(who);
    if (block_size != 4 && block_size != 8 && block_size != 16 && block_size != 32) {
        set_error(w + ": block_size must be 4, 8, 16 or 32");
        return NH_EARG;
    }
    if (use_dst && block_size != 4) {
        set_error(w + ": use_dst needs block_size 4 (transform.py:138-141)");
        return NH_EARG;
    }
    if (check_qp && (qp < 0 || qp > 51)) {
        set_error(w + ": qp outside 0..51");
        return NH_EARG;
    }
    if (nsets < 1 || nsets > NH_MAX_PLANE_SETS) {
        set_error(w + ": nsets outside 1..8");
        return NH_EARG;
    }
    for (int k = 0; k < nsets; ++k) {
        const nh_plane_set& S = sets[k];
        const int64_t planes = (int64_t)S.planes_per_group * S.num_groups;
        if (S.width < 0 || S.height < 0 || S.pitch < S.width || S.planes_per_group < 1 || S.num_groups < 0 ||
            planes > 65535 || S.base < 0 || S.plane_stride < 0 || S.group_stride < 0) {
            set_error(w + ": bad plane set");
            return NH_EARG;
        }
    }
    return NH_OK;
}

}  // namespace nh

using namespace nh;

extern "C" int nh_dequant_inv_planes_n(const void* d_lvl, int lvl_bytes, int16_t* d_res, const nh_plane_set* sets,
                                       int nsets, int block_size, int use_dst, int qp, void* stream) {
    if (!d_lvl || !d_res || !sets) {
        set_error("nh_dequant_inv_planes_n: null argument");
        return NH_EARG;
    }
    NH_TRY(check_rdo_n_args("nh_dequant_inv_planes_n", sets, nsets, block_size, use_dst, qp, false));
    if (lvl_bytes != 2 && lvl_bytes != 4) {
        set_error("nh_dequant_inv_planes_n: lvl_bytes must be 2 (int16) or 4 (int32)");
        return NH_EARG;
    }
    if (((uintptr_t)d_lvl & (uintptr_t)(lvl_bytes - 1)) || ((uintptr_t)d_res & 1)) {
        set_error("nh_dequant_inv_planes_n: buffers must be aligned to their element size");
        return NH_EARG;
    }
    if (block_size == 8) return nh_dequant_inv8x8_planes(d_lvl, lvl_bytes, d_res, sets, nsets, qp, stream);
    const int N = block_size;
    DeqNArgs a{};
    a.lvl = d_lvl;
    a.res = d_res;
    a.log2n = log2_of(N);
    a.dst = use_dst ? 1 : 0;
    bool aligned = !((uintptr_t)d_lvl & 15) && !((uintptr_t)d_res & 15);
    uint64_t wg = 0;
    for (int k = 0; k < nsets; ++k) {
        const nh_plane_set& p = sets[k];
        if ((p.base | p.plane_stride | p.group_stride | p.pitch) & 7) aligned = false;
        DeqNSet& d = a.set[k];
        d.base = p.base;
        d.plane_stride = p.plane_stride;
        d.group_stride = p.group_stride;
        d.pitch = p.pitch;
        d.ppg = p.planes_per_group;
        d.fw = p.width / N * N;
        d.fh = p.height / N * N;
        d.rcols = (d.fw + 31) / 32;
        d.rrows = (d.fh + 31) / 32;
        d.wg_start = (uint32_t)wg;
        wg += (uint64_t)d.rcols * d.rrows * (uint64_t)p.planes_per_group * (uint64_t)p.num_groups;
        if (wg >= (1ull << 31)) {
            set_error("nh_dequant_inv_planes_n: > 2^31 workgroups");
            return NH_EARG;
        }
    }
    for (int k = nsets; k < NH_MAX_PLANE_SETS; ++k) a.set[k].wg_start = 0xffffffffu;
    if (!wg) return NH_OK;
    const int q = qp < 0 ? 0 : (qp > 51 ? 51 : qp);   // quant.py:35
    a.scale = dequant_scale(q % 6);
    a.per = q / 6;
    const hipStream_t s = as_stream(stream);
    const unsigned grid = (unsigned)wg;
    if (lvl_bytes == 2) {
        if (aligned) k_dequant_inv_n<2, true><<<grid, 256, 0, s>>>(a);
        else k_dequant_inv_n<2, false><<<grid, 256, 0, s>>>(a);
    } else {
        if (aligned) k_dequant_inv_n<4, true><<<grid, 256, 0, s>>>(a);
        else k_dequant_inv_n<4, false><<<grid, 256, 0, s>>>(a);
    }
    NH_HIP(hipGetLastError());
    return NH_OK;
}
