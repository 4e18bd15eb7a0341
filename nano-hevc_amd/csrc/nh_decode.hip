// nh_decode.hip -- stage R of the decoder: the mirror of
// the hot path.  Per full 8x8 block of int16 / int32 level planes
//   res = inverse_transform(dequantize_block(level, qp)).astype(np.int16)
// (quant.py:82-123, transform.py:199-238), int16 residual written at the
// block's raster position.  Exact for EVERY level value of the input dtype:
//   * dequantiser: levels inside int16 take one 24-bit mad + shift (|l * scale
//     << max(0, per - 4)| < 2^26, no wrap, the reference's int64 is not needed);
//     any other int32 level takes dequant_i32 (64-bit product and rounding
//     shift, int32 wrap of the result) -- per block, so an int32 plane of
//     encoder levels runs the short form;
//   * inverse pass 1 multiplies the dequantised coefficients themselves (the
//     inverse butterfly multiplies first and adds after): v_mad_i32_i24 when
//     they provably fit signed 24 bits (int16-range levels at QP <= 40:
//     |l| * 256 <= 2^23, tools/decode_bounds.py), the full 32-bit product
//     otherwise; sums wrap mod 2^32 as the reference's int32 accumulators;
//   * inverse pass 2 multiplies (acc + 128) >> 8 of a wrapped int32: always in
//     [-2^23, 2^23), so v_mad_i32_i24 is exact for every input;
//   * astype(int16) keeps the low 16 bits.
// One thread = one block in VGPRs, set lookup, block addressing, cache policy
// and XCD-aware workgroup order as k_fwd8x8_quant (nh_fused8x8.hpp).
#include <hip/hip_runtime.h>
#include <string>
#include "nh_common.hpp"
#include "nh_internal.hpp"
#include "nh_fused8x8.hpp"

namespace nh {

struct DeqParams {
    int32_t scale, per;   // DEQUANT_SCALE[qp % 6], qp / 6 (dequant_i32)
    int32_t dqs, dqsh;    // short form: (l * dqs + dqr) >> dqsh
    uint32_t dqr;
};

// X: the block's levels (int32 bits) in, the residual before astype(int16) out.
// DQ64: levels are any int32; otherwise every level is inside int16.
// P24: every dequantised coefficient fits signed 24 bits (never with DQ64).
template <bool DQ64, bool P24>
__device__ __forceinline__ void dq_inv8_block(uint32_t (&X)[8][8], const DeqParams& d, uint32_t dqr_v) {
    static_assert(!(DQ64 && P24), "24-bit pass 1 needs bounded levels");
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (DQ64) {
                X[i][j] = (uint32_t)dequant_i32((int32_t)X[i][j], d.scale, d.per);
            } else {
                int32_t r;
                asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(X[i][j]), "s"(d.dqs), "v"(dqr_v));
                X[i][j] = (uint32_t)(r >> d.dqsh);
            }
        }
    // pass 1: columns, temp[i][j] = (sum_k T[k][i] * c[k][j] + 128) >> 8  (transform.py:221-227)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t y[8], x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) y[k] = X[k][j];
        if constexpr (P24) inv_dct<8, Mul24>(y, x, 128u);
        else inv_dct<8, MulWrap>(y, x, 128u);
#pragma unroll
        for (int i = 0; i < 8; ++i) X[i][j] = (uint32_t)((int32_t)x[i] >> 8);
    }
    // pass 2: rows, res[i][j] = (sum_k temp[i][k] * T[k][j] + 128) >> 8  (transform.py:230-236)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t x[8];
        inv_dct<8, Mul24>(X[i], x, 128u);
#pragma unroll
        for (int j = 0; j < 8; ++j) X[i][j] = (uint32_t)((int32_t)x[j] >> 8);
    }
}

// LB: bytes per level (2 / 4).  ALIGNED: 16-byte row accesses (base, pitch and
// strides multiples of 8 elements, buffers 16-B aligned); otherwise one
// element per access.  P24: the host's bound for int16-range levels (QP <= 40).
template <int LB, bool ALIGNED, bool P24, int WAVES>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVES)))
k_dequant_inv8x8(Fused8Args a, DeqParams d) {
    const uint32_t wid = xcd_eighths(blockIdx.x, gridDim.x);
    SetDev S;
    select_set(a, S, wid);
    uint32_t dqr_v = d.dqr;
    asm volatile("" : "+v"(dqr_v));
    const uint32_t b = (wid - S.wg_start) * 256u + threadIdx.x;
    if (b >= S.nblocks) return;
    const int64_t off = block_offset(S, b);
    uint32_t X[8][8];
    if constexpr (LB == 2) {
        const int16_t* src = a.in + off;
        if constexpr (ALIGNED) {
            v4i raw[8];
            load_block<1>(src, S.pitch, raw);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int w[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    X[i][2 * m] = (uint32_t)(int32_t)(int16_t)(w[m] & 0xffff);
                    X[i][2 * m + 1] = (uint32_t)(w[m] >> 16);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) X[i][j] = (uint32_t)(int32_t)src[(int64_t)i * S.pitch + j];
        }
    } else {
        const int32_t* src = reinterpret_cast<const int32_t*>(a.in) + off;
        if constexpr (ALIGNED) {
            v4i raw[8][2];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                raw[i][0] = __builtin_nontemporal_load((const v4i*)(src + (int64_t)i * S.pitch));
                raw[i][1] = __builtin_nontemporal_load((const v4i*)(src + (int64_t)i * S.pitch + 4));
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                X[i][0] = (uint32_t)raw[i][0].x; X[i][1] = (uint32_t)raw[i][0].y;
                X[i][2] = (uint32_t)raw[i][0].z; X[i][3] = (uint32_t)raw[i][0].w;
                X[i][4] = (uint32_t)raw[i][1].x; X[i][5] = (uint32_t)raw[i][1].y;
                X[i][6] = (uint32_t)raw[i][1].z; X[i][7] = (uint32_t)raw[i][1].w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) X[i][j] = (uint32_t)src[(int64_t)i * S.pitch + j];
        }
    }
    if constexpr (LB == 2) {
        dq_inv8_block<false, P24>(X, d, dqr_v);
    } else {
        uint32_t wide = 0;   // some level outside int16
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) wide |= (X[i][j] + 32768u) >> 16;
        if (!wide) dq_inv8_block<false, P24>(X, d, dqr_v);
        else dq_inv8_block<true, false>(X, d, dqr_v);
    }
    int16_t* dst = a.out + off;
    if constexpr (ALIGNED) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int w[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) w[m] = (int)__builtin_amdgcn_perm(X[i][2 * m + 1], X[i][2 * m], 0x05040100u);
            st16<1>(dst + (int64_t)i * S.pitch, v4i{w[0], w[1], w[2], w[3]});
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[(int64_t)i * S.pitch + j] = (int16_t)(uint16_t)X[i][j];
    }
}

template <int LB, bool ALIGNED>
static void launch_dequant_inv8x8(bool p24, uint32_t wg, hipStream_t s, const Fused8Args& a, const DeqParams& d) {
    // occupancy targets: the largest without spills
    constexpr int W = LB == 2 ? 5 : 3;
    if (p24) k_dequant_inv8x8<LB, ALIGNED, true, W><<<wg, 256, 0, s>>>(a, d);
    else k_dequant_inv8x8<LB, ALIGNED, false, W><<<wg, 256, 0, s>>>(a, d);
}

}  // namespace nh

using namespace nh;

extern "C" int nh_dequant_inv8x8_planes(const void* d_lvl, int lvl_bytes, int16_t* d_res, const nh_plane_set* sets,
                                        int nsets, int qp, void* stream) {
    if (!d_lvl || !d_res || !sets) {
        set_error("nh_dequant_inv8x8_planes: null argument");
        return NH_EARG;
    }
    if (nsets < 1 || nsets > NH_MAX_PLANE_SETS) {
        set_error("nh_dequant_inv8x8_planes: nsets must be 1.." + std::to_string(NH_MAX_PLANE_SETS));
        return NH_EARG;
    }
    if (lvl_bytes != 2 && lvl_bytes != 4) {
        set_error("nh_dequant_inv8x8_planes: lvl_bytes must be 2 (int16) or 4 (int32)");
        return NH_EARG;
    }
    if (((uintptr_t)d_lvl & (uintptr_t)(lvl_bytes - 1)) || ((uintptr_t)d_res & 1)) {
        set_error("nh_dequant_inv8x8_planes: buffers must be aligned to their element size");
        return NH_EARG;
    }
    Fused8Args a{};
    a.in = static_cast<const int16_t*>(d_lvl);   // int32 levels: the kernel reinterprets
    a.out = d_res;
    a.nsets = nsets;
    bool aligned = !((uintptr_t)d_lvl & 15) && !((uintptr_t)d_res & 15);
    uint64_t wg = 0, blk = 0;
    for (int k = 0; k < nsets; ++k) {
        const nh_plane_set& p = sets[k];
        if (p.width < 1 || p.height < 1 || p.pitch < p.width || p.planes_per_group < 1 || p.num_groups < 0) {
            set_error("nh_dequant_inv8x8_planes: plane set must have positive sizes and pitch >= width");
            return NH_EARG;
        }
        if ((p.base | p.plane_stride | p.group_stride | p.pitch) & 7) aligned = false;
        const uint64_t bpr = p.width / 8, rows = p.height / 8;
        const uint64_t bpp = bpr * rows, nb = bpp * (uint64_t)p.planes_per_group * (uint64_t)p.num_groups;
        if (nb >= (1ull << 31)) {
            set_error("nh_dequant_inv8x8_planes: > 2^31 blocks per set");
            return NH_EARG;
        }
        SetDev& d = a.set[k];
        d.base = p.base;
        d.plane_stride = p.plane_stride;
        d.group_stride = p.group_stride;
        d.pitch = p.pitch;
        d.nblocks = (uint32_t)nb;
        d.wg_start = (uint32_t)wg;
        d.bpp = make_fastdiv(bpp ? (uint32_t)bpp : 1);
        d.bpr = make_fastdiv(bpr ? (uint32_t)bpr : 1);
        d.ppg = make_fastdiv((uint32_t)p.planes_per_group);
        d.blk0 = (uint32_t)blk;
        blk += nb;
        wg += (nb + 255) / 256;
    }
    for (int k = nsets; k < NH_MAX_PLANE_SETS; ++k) a.set[k].wg_start = 0xffffffffu;
    if (wg >= (1ull << 31) || blk >= (1ull << 32)) {
        set_error("nh_dequant_inv8x8_planes: > 2^31 workgroups");
        return NH_EARG;
    }
    if (!wg) return NH_OK;
    const int q = qp < 0 ? 0 : (qp > 51 ? 51 : qp);   // quant.py:35
    DeqParams d;
    d.scale = dequant_scale(q % 6);
    d.per = q / 6;
    d.dqs = d.per < 4 ? d.scale : d.scale << (d.per - 4);
    d.dqr = d.per < 4 ? 1u << (3 - d.per) : 0u;
    d.dqsh = d.per < 4 ? 4 - d.per : 0;
    // int16-range levels dequantise into signed 24 bits iff 32768 * dqs <= 2^23: QP <= 40
    const bool p24 = d.dqs <= 256;
    hipStream_t s = as_stream(stream);
    const uint32_t g = (uint32_t)wg;
    if (lvl_bytes == 2) {
        if (aligned) launch_dequant_inv8x8<2, true>(p24, g, s, a, d);
        else launch_dequant_inv8x8<2, false>(p24, g, s, a, d);
    } else {
        if (aligned) launch_dequant_inv8x8<4, true>(p24, g, s, a, d);
        else launch_dequant_inv8x8<4, false>(p24, g, s, a, d);
    }
    NH_HIP(hipGetLastError());
    return NH_OK;
}
