"""GPU parity: the HIP path (through the C ABI) against the reference's recorded
outputs (tests/golden) and the CPU restatement (oracle/) on seeded inputs.
Bar: bit-exact (integer work).  Run with ``pytest -m gpu`` on an MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from natural import natural_residual  # noqa: E402
from block_checks import (check_chain_config1, check_intra_golden, check_metrics_golden,  # noqa: E402
                          check_quant_golden, check_transforms_golden)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def nh():
    import nano_hevc
    from nano_hevc import _lib
    assert _lib.device_count() > 0, "no HIP device: the gpu tests need an MI355X"
    return nano_hevc


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------ per-block drop-in path

@pytest.mark.parametrize("key,n,dst", [("n4_dst", 4, True), ("n4_dct", 4, False), ("n8_dct", 8, False),
                                       ("n16_dct", 16, False), ("n32_dct", 32, False)])
def test_shim_transforms_golden(nh, golden, key, n, dst):
    check_transforms_golden(nh, golden("transform.npz"), key, n, dst)


def test_shim_quant_golden(nh, golden):
    check_quant_golden(nh, golden("quant.npz"))


@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_shim_intra_golden(nh, golden, n):
    check_intra_golden(nh, golden("intra.npz"), n)


def test_shim_quirks_and_elementwise(nh, golden):
    g = golden("intra.npz")
    t, l = g["quirk_top"], g["quirk_left"]
    assert np.array_equal(nh.intra_angular_predict(t, l, 77, 0, 4), g["quirk_ang0"])
    assert np.array_equal(nh.intra_angular_predict(t, l, 77, 1, 4), g["quirk_ang1"])
    assert np.array_equal(nh.intra_angular_predict(t, l, 77, -5, 4), g["quirk_angm5"])
    assert np.array_equal(nh.intra_dc_predict_4x4(t, l), g["quirk_dc4"])
    assert np.array_equal(nh.intra_dc_predict(t, l, 4), g["quirk_dc4_len9"])
    assert np.array_equal(nh.residual_block(g["rr_a"], g["rr_b"]), g["rr_res"])
    assert np.array_equal(nh.reconstruct_block(g["rr_a"], g["rr_b"]), g["rr_rec"])
    for bd in [1, 8, 10, 12, 16, 40, 63]:
        assert np.array_equal(nh.clip_to_pixel_range(g["clip_in"], bd), g[f"clip_bd{bd}"]), bd
    # broadcasting + dtype casts of residual_block (intra.py:65-67)
    assert np.array_equal(nh.residual_block(np.array([[1, 2]], np.uint8), np.array([[300]], np.int32)), [[-299, -298]])


def test_shim_chain_config1(nh, golden):
    """Config 1: the README / test_quant.py:283-322 chain, bit-exact per stage."""
    check_chain_config1(nh, golden("chain.npz"))


def test_shim_reference_known_answers(nh):
    """Known answers held by the reference's own tests, via the drop-in."""
    assert np.all(nh.intra_dc_predict_4x4(np.array([102, 98, 100, 101]), np.array([103, 102, 101, 99])) == 101)
    p = nh.intra_planar_predict(np.zeros(4, np.int16), np.zeros(4, np.int16), 255, 255, 4)
    assert p[0, 0] == 64 and p[3, 3] == 255                                    # test_intra_planar.py:56-76
    top = np.array([0, 10, 20, 30, 40, 50, 60, 70, 80], np.int16)
    left = np.array([0, 5, 5, 5, 5, 5, 5, 5, 5], np.int16)
    exp18 = np.array([[0, 10, 20, 30], [0, 0, 10, 20], [5, 0, 0, 10], [5, 5, 0, 0]])
    assert np.array_equal(nh.intra_angular_predict(top, left, 0, 18, 4), exp18)   # test_intra_angular.py:69-85
    for m in range(2, 35):
        assert np.all(nh.intra_angular_predict(np.full(9, 128, np.int16), np.full(9, 128, np.int16), 128, m, 4) == 128)
    assert np.array_equal(nh.clip_to_pixel_range(np.array([[-10, 0, 128, 255, 300]], np.int16)), [[0, 0, 128, 255, 255]])
    lv = np.array([[10, 0, 0, 0], [0, 5, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], np.int32)
    assert nh.quant.count_nonzero(lv) == 3 and nh.quant.is_all_zero(np.zeros((4, 4), np.int32))
    assert not nh.quant.is_all_zero(np.array([[1, 0], [0, 0]], np.int32))
    assert nh.quant.quantize(np.array([-32768], np.int16), 0, 4)[0] == 13107       # np.abs int16 wrap


def test_shim_estimate_bits(nh):
    rng = np.random.default_rng(5)
    for n in [1, 7, 8, 16, 64, 129, 1024, 4096]:
        lv = rng.integers(-3000, 3000, size=n).astype(np.int32)
        lv[rng.random(n) < 0.5] = 0
        a = np.abs(lv)
        exp = int(np.sum(np.log2(a + 1) + (a > 0) * 2))     # quant.py:166-167 (numpy as checker)
        assert nh.quant.estimate_bits(lv) == exp, n
        assert nh.quant.count_nonzero(lv) == int(np.count_nonzero(lv))


@pytest.mark.parametrize("n", [4, 32, 96, 256])
def test_shim_small_and_staged_forms(nh, n):
    """The per-block protocol's two forms (nh_blocks.hip BlockCall): inputs up to
    3 KB run as one kernel-argument launch, larger arrays through one staged
    H2D / D2H pair.  n = 4, 32 cross the threshold per function; both forms
    against the oracle, including an error raised from each form."""
    rng = np.random.default_rng(n)
    a = rng.integers(-300, 300, (n, n)).astype(np.int16)
    b = rng.integers(-300, 300, (n, n)).astype(np.int16)
    assert np.array_equal(nh.residual_block(a, b), O.residual(a, b))
    assert np.array_equal(nh.reconstruct_block(a, b), O.reconstruct(a, b))
    assert np.array_equal(nh.clip_to_pixel_range(a.astype(np.int32) * 3, 8), O.clip(a.astype(np.int32) * 3, 8))
    c = rng.integers(-40000, 40000, (n, n)).astype(np.int32)
    lv = nh.quantize(c, 12, min(n, 32))
    assert np.array_equal(lv, O.quantize(c, 12, min(n, 32)))
    assert np.array_equal(nh.dequantize(lv, 12, 4), O.dequantize(lv, 12, 4))
    assert nh.quant.count_nonzero(lv) == int(np.count_nonzero(lv))
    assert nh.residual_energy(a) == int(np.sum(a.astype(np.int64) ** 2))
    assert nh.sad(a, b) == int(np.sum(np.abs(a.astype(np.int32) - b)))
    top = rng.integers(0, 256, n).astype(np.int16)
    left = rng.integers(0, 256, n).astype(np.int16)
    assert np.array_equal(nh.intra_planar_predict(top, left, int(top[-1]), int(left[-1]), n),
                          O.intra_planar(top, left, int(top[-1]), int(left[-1]), n))
    with pytest.raises(IndexError):   # short left reference: raised from either form
        nh.intra_planar_predict(top, left[:n // 2], 1, 1, n)


def test_staging_contexts_do_not_grow(nh, torch_dev):
    """Per-device contexts of the per-block path: constant footprint over many
    calls, freed by nh_release_staging and re-created once (VERDICT r1 weak 7:
    the old single context leaked its buffers on every device switch)."""
    import ctypes as C
    from nano_hevc import _lib
    lib = _lib.load()
    dev = torch_dev.cuda.current_device()
    held = C.c_int64(0)

    def footprint():
        assert lib.nh_staging_bytes(dev, C.byref(held)) == 0
        return held.value

    x = np.arange(64, dtype=np.int16).reshape(8, 8)
    big = np.ones((128, 128), np.int16)
    nh.residual_block(x, x)
    nh.residual_block(big, big)   # staged form: grows once to its cap
    f0 = footprint()
    assert f0 > 0
    for _ in range(300):
        nh.residual_block(x, x)
        nh.residual_block(big, big)
    assert footprint() == f0
    torch_dev.cuda.synchronize()
    free0 = torch_dev.cuda.mem_get_info(dev)[0]
    for _ in range(20):           # release / re-create cycles leave no device memory behind
        assert lib.nh_release_staging() == 0
        assert footprint() == 0
        assert np.array_equal(nh.residual_block(big, x[:1, :1]), big - x[0, 0])
        assert footprint() == f0
    assert torch_dev.cuda.mem_get_info(dev)[0] >= free0 - (8 << 20)


# ------------------------------------------------------------------ batched device path

@pytest.mark.parametrize("n,dst", [(4, True), (4, False), (8, False), (16, False), (32, False)])
def test_batch_transforms_vs_oracle(nh, torch_dev, n, dst):
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(n + dst)
    x = rng.integers(-2**31, 2**31, size=(97, n, n), dtype=np.int64).astype(np.int32)
    x[:40] = rng.integers(-255, 256, size=(40, n, n))
    d = torch.from_numpy(x).cuda()
    f = gpu.fwd_transform_batch(d, dst).cpu().numpy()
    i = gpu.inv_transform_batch(d, dst).cpu().numpy()
    for b in range(x.shape[0]):
        assert np.array_equal(f[b], O.forward_transform(x[b], dst)), b
        assert np.array_equal(i[b], O.inverse_transform(x[b], dst)), b


def test_batch_quant_vs_oracle(nh, torch_dev):
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(3)
    c = rng.integers(-2**31, 2**31, size=5000, dtype=np.int64).astype(np.int32)
    c[:2000] = rng.integers(-3000, 3000, size=2000)
    c[:3] = [-2**31, 2**31 - 1, 0]
    d = torch.from_numpy(c).cuda()
    for qp in [0, 7, 22, 32, 45, 51]:
        for lg in [2, 3, 4, 5]:
            for intra in (True, False):
                got = gpu.quant_batch(d, qp, lg, intra).cpu().numpy()
                assert np.array_equal(got, O.quantize(c, qp, 1 << lg, intra)), (qp, lg, intra)
        assert np.array_equal(gpu.dequant_batch(d, qp).cpu().numpy(), O.dequantize(c, qp)), qp


def _plane_gpu(torch, plane, qp=32, intra=True, variant=0):
    from nano_hevc import gpu
    h, w = plane.shape
    d = torch.from_numpy(np.ascontiguousarray(plane)).cuda()
    out = torch.full_like(d, 0x5555)
    gpu.fwd8x8_quant(d, [gpu.plane_set(0, w, h, w)], qp, intra, out=out, variant=variant)
    return out.cpu().numpy()


def test_fused8x8_golden_planes(nh, torch_dev, golden):
    g = golden("planes.npz")
    out = _plane_gpu(torch_dev, g["p2_small_in"])
    assert np.array_equal(out, g["p2_small_lvl"])
    out = _plane_gpu(torch_dev, g["p2_edge_in"], qp=0)
    assert np.array_equal(out, g["p2_edge_lvl"])


def test_fused8x8_1080p_hash(nh, torch_dev):
    """reference levels of a seeded 1080p plane, by sha256."""
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    rng = np.random.default_rng(20260)
    plane = rng.integers(-255, 256, size=(1080, 1920)).astype(np.int16)
    out = _plane_gpu(torch_dev, plane, 32)
    assert hashlib.sha256(out.tobytes()).hexdigest() == man["cfg2_1080p_qp32_seed20260_levels_sha256"]


@pytest.mark.parametrize("qp,intra", [(0, True), (22, True), (32, True), (32, False), (51, True), (-4, True), (70, False)])
def test_fused8x8_full_int16_range_vs_oracle(nh, torch_dev, qp, intra):
    """Every int16 input (incl. +-32767/-32768 blocks) is exact: the 24-bit mads
    and the single-mad quantizer are proved for the whole int16 range."""
    rng = np.random.default_rng(qp + 100)
    plane = rng.integers(-32768, 32768, size=(136, 264)).astype(np.int16)
    plane[:8, :8] = 32767
    plane[:8, 8:16] = -32768
    plane[8:16, :8] = np.where(np.indices((8, 8)).sum(0) % 2, 32767, -32768)
    plane[8:16, 8:16] = np.where(np.indices((8, 8))[0] < 4, -32768, 32767)
    exp = O.fwd8x8_quant_plane(plane, qp, intra)
    got = _plane_gpu(torch_dev, plane, qp, intra)
    assert np.array_equal(got, exp)
    assert np.array_equal(_plane_gpu(torch_dev, plane, qp, intra, variant=1), got)


def test_fused8x8_partial_blocks_untouched(nh, torch_dev):
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(9)
    plane = rng.integers(-255, 256, size=(21, 40)).astype(np.int16)   # 21 rows: last 5 rows partial
    d = torch.from_numpy(plane).cuda()
    out = torch.full_like(d, 1234)
    gpu.fwd8x8_quant(d, [gpu.plane_set(0, 40, 21, 40)], 32, True, out=out)
    o = out.cpu().numpy()
    assert np.all(o[16:] == 1234)
    assert np.array_equal(o[:16], O.fwd8x8_quant_plane(plane[:16], 32))


def test_fused8x8_4k_yuv420_stream_vs_oracle(nh, torch_dev):
    """The metric's workload shape: 4K YUV420 frames back to back, one launch
    over both plane sets (Y, U+V), every block compared with the oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H = 3, 3840, 2160
    fe = gpu.yuv420_frame_elems(W, H)
    rng = np.random.default_rng(77)
    buf = rng.integers(-255, 256, size=F * fe).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    sets = gpu.yuv420_plane_sets(F, W, H)
    out = gpu.fwd8x8_quant(d, sets, 32, True).cpu().numpy()
    for f in range(F):
        base = f * fe
        y = buf[base:base + W * H].reshape(H, W)
        assert np.array_equal(out[base:base + W * H].reshape(H, W), O.fwd8x8_quant_plane(y, 32)), f
        for c in range(2):
            o = base + W * H + c * (W // 2) * (H // 2)
            p = buf[o:o + (W // 2) * (H // 2)].reshape(H // 2, W // 2)
            assert np.array_equal(out[o:o + p.size].reshape(p.shape), O.fwd8x8_quant_plane(p, 32)), (f, c)


def test_fused8x8_natural_residual_stream_vs_oracle(nh, torch_dev):
    """D-1 (b): "natural" residuals (gradient + noise frames minus the open-loop
    DC prediction) of a 4K YUV420 stream, every block against the oracle, at
    QP 22 and 32 (intra) and QP 37 (inter)."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H = 2, 3840, 2160
    rng = np.random.default_rng(2024)
    planes = []
    for f in range(F):
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            src = np.clip(40 + (3 * xx + 2 * yy + 13 * f) % 170 + (xx // 97) * 5 + rng.integers(-12, 13, (ph, pw)),
                          0, 255)
            planes.append(natural_residual(src))
    buf = np.concatenate([p.reshape(-1) for p in planes])
    d = torch.from_numpy(buf).cuda()
    sets = gpu.yuv420_plane_sets(F, W, H)
    for qp, intra in ((22, True), (32, True), (37, False)):
        out = gpu.fwd8x8_quant(d, sets, qp, intra).cpu().numpy()
        o = 0
        for p in planes:
            assert np.array_equal(out[o:o + p.size].reshape(p.shape), O.fwd8x8_quant_plane(p, qp, intra)), (qp, o)
            o += p.size


# ------------------------------------------------------------------ config 3 / config 4 drivers

def test_intra_rdo_golden(nh, torch_dev, golden):
    """Config 3 vs planes recorded from the reference functions (make_golden.py)."""
    torch = torch_dev
    from nano_hevc import gpu
    g = golden("planes.npz")
    for k, qp in (("p3", 32), ("p3b", 22)):
        m, l, r, sse = gpu.intra_rdo_plane(torch.from_numpy(g[f"{k}_src"]).cuda(), qp)
        h8, w8 = g[f"{k}_modes"].shape
        assert np.array_equal(m.cpu().numpy(), g[f"{k}_modes"]), k
        assert np.array_equal(l.cpu().numpy()[:h8 * 8, :w8 * 8], g[f"{k}_lvl"][:h8 * 8, :w8 * 8]), k
        assert np.array_equal(r.cpu().numpy()[:h8 * 8, :w8 * 8], g[f"{k}_rec"][:h8 * 8, :w8 * 8]), k
        assert int(sse.item()) == int(g[f"{k}_sse"]), k


@pytest.mark.parametrize("h,w,kind", [(64, 96, "natural"), (48, 40, "noise"), (72, 64, "int16"), (56, 72, "mixed"),
                                      (40, 60, "noise")])
def test_intra_rdo_vs_oracle(nh, torch_dev, h, w, kind):
    """noise: the packed 16-bit chain at its extremes (residuals +-255); int16:
    the 32-bit chain; mixed: 8-bit blocks whose left / top neighbours are not
    8-bit (wide = 2: the 32-bit chain with the 32-bit SSE); width 60: rows not
    16-B aligned (the winners' per-sample stores instead of 16-B rows)."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(h * w)
    if kind == "natural":
        yy, xx = np.mgrid[0:h, 0:w]
        src = np.clip(40 + 3 * xx - yy + rng.integers(-10, 11, size=xx.shape), 0, 255).astype(np.int16)
    elif kind == "noise":
        src = rng.integers(0, 256, size=(h, w)).astype(np.int16)
    elif kind == "mixed":
        src = rng.integers(0, 256, size=(h, w)).astype(np.int16)
        src[:, 15::16] = rng.integers(256, 400, size=src[:, 15::16].shape)    # a right column every other block
        src[23::24, :] = rng.integers(-300, 0, size=src[23::24, :].shape)     # a bottom row every third block row
    else:   # arbitrary int16 samples: exercises the int16 wraps of residual/recon (D8-like) and 24-bit bounds
        src = rng.integers(-32768, 32768, size=(h, w)).astype(np.int16)
    for qp in (0, 32, 51):
        m, l, r, sse = gpu.intra_rdo_plane(torch.from_numpy(src).cuda(), qp)
        em, el, er, esse = O.intra_rdo_plane(src, qp)
        assert np.array_equal(m.cpu().numpy(), em), (kind, qp)
        assert np.array_equal(l.cpu().numpy(), el), (kind, qp)
        assert np.array_equal(r.cpu().numpy(), er), (kind, qp)
        assert int(sse.item()) == esse


@pytest.mark.parametrize("qp,pad", [(32, 0), (7, 24), (51, 8)])
def test_intra_rdo_planes_equal_per_plane(nh, torch_dev, qp, pad):
    """intra_rdo_planes (plane sets, one launch pair per set) equals intra_rdo_plane
    plane by plane: a 3-frame YUV420 stream with a padded frame stride and a base
    offset, partial blocks at the right / bottom edges, one int16-extreme frame
    (its groups go to the general fallback launch)."""
    torch = torch_dev
    from nano_hevc import gpu
    W, H, F, base = 104, 76, 3, 16
    rng = np.random.default_rng(qp * 10 + pad)
    fe = gpu.yuv420_frame_elems(W, H)
    fs = fe + pad
    buf = np.zeros(base + F * fs, np.int16)
    planes = []
    for f in range(F):
        off = base + f * fs
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = np.clip(40 + (3 * xx + 2 * yy + 9 * f) % 170 + rng.integers(-15, 16, (ph, pw)), 0, 255)
            if f == 1:
                p = rng.integers(-32768, 32768, (ph, pw))
            buf[off:off + ph * pw] = p.reshape(-1)
            planes.append((off, ph, pw))
            off += ph * pw
    d = torch.from_numpy(buf).cuda()
    m, l, r, s = gpu.intra_rdo_planes(d, gpu.yuv420_plane_sets(F, W, H, fs, base), qp)
    m, l, r, s = m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()
    order = [3 * f for f in range(F)] + [3 * f + c for f in range(F) for c in (1, 2)]
    mo = 0
    for k, pi in enumerate(order):
        off, ph, pw = planes[pi]
        em, el, er, es = gpu.intra_rdo_plane(d[off:off + ph * pw].view(ph, pw), qp)
        n = (ph // 8) * (pw // 8)
        assert np.array_equal(m[mo:mo + n], em.cpu().numpy().reshape(-1)), (k, pi)
        mo += n
        assert np.array_equal(l[off:off + ph * pw].reshape(ph, pw), el.cpu().numpy()), (k, pi)
        assert np.array_equal(r[off:off + ph * pw].reshape(ph, pw), er.cpu().numpy()), (k, pi)
        assert int(s[k]) == int(es.item()), (k, pi)


def test_intra_rdo_every_qp_vs_oracle(nh, torch_dev):
    """The packed chain at every QP 0..51 on 8-bit extremes (0 / 255 checkerboards and
    noise: the largest coefficients and levels, where the packed dequantization's
    int16 bound is tightest, tools/packed_bounds.py rdo8_dequant_bounds)."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(52)
    h, w = 32, 64
    yy, xx = np.mgrid[0:h, 0:w]
    src = rng.integers(0, 256, size=(h, w))
    src[:, :24] = 255 * ((xx[:, :24] + yy[:, :24]) % 2)          # checkerboards
    src[:16, 24:40] = 255 * ((xx[:16, 24:40] // 2 + yy[:16, 24:40]) % 2)
    src = src.astype(np.int16)
    d = torch.from_numpy(src).cuda()
    for qp in range(52):
        m, l, r, sse = gpu.intra_rdo_plane(d, qp)
        em, el, er, esse = O.intra_rdo_plane(src, qp)
        assert np.array_equal(m.cpu().numpy(), em), qp
        assert np.array_equal(l.cpu().numpy(), el), qp
        assert np.array_equal(r.cpu().numpy(), er), qp
        assert int(sse.item()) == esse, qp


def test_tu_pipeline_golden(nh, torch_dev, golden):
    torch = torch_dev
    from nano_hevc import gpu
    g = golden("planes.npz")
    l, r, t = gpu.tu_pipeline_plane(torch.from_numpy(g["p4y_src"]).cuda(), 32, 0, 1234, 32, True)
    assert np.array_equal(t.cpu().numpy(), g["p4y_tu"])
    assert np.array_equal(l.cpu().numpy(), g["p4y_lvl"]) and np.array_equal(r.cpu().numpy(), g["p4y_rec"])
    l, r, t = gpu.tu_pipeline_plane(torch.from_numpy(g["p4u_src"]).cuda(), 16, 1, 1234, 32, False)
    assert np.array_equal(t.cpu().numpy(), g["p4u_tu"])
    assert np.array_equal(l.cpu().numpy(), g["p4u_lvl"]) and np.array_equal(r.cpu().numpy(), g["p4u_rec"])


@pytest.mark.parametrize("h,w,ctb,luma,seed", [(136, 200, 32, True, 7), (68, 100, 16, False, 7), (64, 64, 32, True, 99),
                                                 (132, 196, 32, True, 5)])   # pitch % 8 != 0: butterfly 32x32
def test_tu_pipeline_vs_oracle_and_bands(nh, torch_dev, h, w, ctb, luma, seed):
    """Whole plane, then the same plane as CTU-row bands (the multi-GPU shard
    unit): bands must tile the plane and agree with the oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(seed + h)
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.clip(120 + xx - 2 * yy + rng.integers(-25, 26, size=xx.shape), 0, 255).astype(np.int16)
    d = torch.from_numpy(src).cuda()
    for qp in (22, 37):
        l, r, t = gpu.tu_pipeline_plane(d, ctb, 0 if luma else 1, seed, qp, luma)
        el, er, et = O.tu_pipeline_plane(src, ctb, 0 if luma else 1, seed, qp, luma)
        assert np.array_equal(t.cpu().numpy(), et) and np.array_equal(l.cpu().numpy(), el)
        assert np.array_equal(r.cpu().numpy(), er)
        rows = (h + ctb - 1) // ctb
        lb = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        rb = torch.zeros((h, w), dtype=torch.int16, device="cuda")
        tb = torch.zeros((h // 4, w // 4), dtype=torch.uint8, device="cuda")
        for r0 in range(0, rows, 2):
            gpu.tu_pipeline_plane(d, ctb, 0 if luma else 1, seed, qp, luma, r0, r0 + 2, lvl=lb, rec=rb, tu=tb)
        assert np.array_equal(lb.cpu().numpy(), el) and np.array_equal(rb.cpu().numpy(), er)


@pytest.mark.parametrize("world", [2, 8])
def test_fused8x8_rank_layouts_vs_oracle(nh, torch_dev, world):
    """The multi-GPU shard layout (nano_hevc/shard.py): every rank's local buffer
    (up to 6 plane sets of different band heights) through one launch; the
    scattered-back levels equal the oracle on the full frames."""
    torch = torch_dev
    from nano_hevc import gpu, shard
    w, h, n = 256, 416, 2 * world            # 13 CTU rows -> uneven bands
    fe = gpu.yuv420_frame_elems(w, h)
    rng = np.random.default_rng(world)
    frames = [rng.integers(-255, 256, size=fe).astype(np.int16) for _ in range(n)]
    back = [np.zeros_like(f) for f in frames]
    for r in range(world):
        L = shard.rank_layout(r, world, n, w, h)
        loc = np.zeros(L.total_elems, np.int16)
        shard.fill_from_frames(L, frames, loc)
        d = torch.from_numpy(loc).cuda()
        out = gpu.fwd8x8_quant(d, L.plane_sets(gpu), 32, True)
        shard.scatter_to_frames(L, out.cpu().numpy(), back)
    cw, ch = w // 2, h // 2
    for f, fr in enumerate(frames):
        exp = np.concatenate([O.fwd8x8_quant_plane(fr[:w * h].reshape(h, w), 32).ravel(),
                              O.fwd8x8_quant_plane(fr[w * h:w * h + cw * ch].reshape(ch, cw), 32).ravel(),
                              O.fwd8x8_quant_plane(fr[w * h + cw * ch:].reshape(ch, cw), 32).ravel()])
        assert np.array_equal(back[f], exp), f


def test_metrics_golden(nh, golden):
    """metrics.py:7-48 through the device reductions vs the reference's values."""
    check_metrics_golden(nh, golden("metrics.npz"))


def test_sse_i16_device(nh, torch_dev):
    torch = torch_dev
    from nano_hevc import _lib
    import ctypes as C
    rng = np.random.default_rng(2)
    a = rng.integers(-32768, 32768, size=1 << 20).astype(np.int16)
    b = rng.integers(-32768, 32768, size=1 << 20).astype(np.int16)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().nh_sse_i16(da.data_ptr(), db.data_ptr(), a.size, out.data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert int(out.item()) == int(np.sum((a.astype(np.int64) - b) ** 2))


# ------------------------------------------------------------------ config 5 (32x32, MFMA vs butterfly)

def test_probe_mfma_i8_lane_maps(nh, torch_dev):
    """The i8 32x32x32 operand/accumulator lane maps the config-5 kernel relies on,
    checked with exact integer data and an asymmetric B."""
    torch = torch_dev
    from nano_hevc import _lib
    import ctypes as C
    rng = np.random.default_rng(8)
    a = rng.integers(-128, 128, size=(32, 32)).astype(np.int8)
    b = rng.integers(-128, 128, size=(32, 32)).astype(np.int8)
    b[0, :] = np.arange(32)          # asymmetric rows/cols
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dd = torch.zeros((32, 32), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().nh_probe_mfma_i8(da.data_ptr(), db.data_ptr(), dd.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(dd.cpu().numpy(), a.astype(np.int32) @ b.astype(np.int32))


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_tc32_golden(nh, torch_dev, golden, variant):
    """Config 5 vs the reference-composed golden plane, incl. the reference's Y-PSNR."""
    torch = torch_dev
    from nano_hevc import gpu
    g = golden("cfg5.npz")
    src = g["p5_src"]
    for qp in (22, 37):
        l, r = gpu.tc32_plane(torch.from_numpy(src).cuda(), qp, variant)
        l, r = l.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(l, g[f"p5_lvl_qp{qp}"]) and np.array_equal(r, g[f"p5_rec_qp{qp}"]), qp
        assert nh.psnr(src[:64, :96].astype(np.uint8), r[:64, :96].astype(np.uint8)) == g[f"p5_psnr_qp{qp}"]


@pytest.mark.parametrize("kind", ["natural", "noise", "int16"])
def test_tc32_mfma_equals_butterfly_and_oracle(nh, torch_dev, kind):
    """int16-extreme planes force the 3-part int8 split in every MFMA stage (and
    variant 1's wide fix-up); 8-bit planes take variant 1's f16 chain."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(len(kind))
    h, w = 96, 160
    if kind == "natural":
        yy, xx = np.mgrid[0:h, 0:w]
        src = np.clip(60 + xx + yy // 2 + rng.integers(-15, 16, size=xx.shape), 0, 255).astype(np.int16)
    elif kind == "noise":
        src = rng.integers(0, 256, size=(h, w)).astype(np.int16)
    else:
        src = rng.integers(-32768, 32768, size=(h, w)).astype(np.int16)
    d = torch.from_numpy(src).cuda()
    for qp in (0, 30, 51):
        el, er = O.tc32_plane(src, qp)
        for v in (0, 1, 2):
            l, r = gpu.tc32_plane(d, qp, v)
            assert np.array_equal(l.cpu().numpy(), el), (kind, qp, v)
            assert np.array_equal(r.cpu().numpy(), er), (kind, qp, v)


def test_tc32_fixup_walks_every_marked_block(nh, torch_dev):
    """Variant 1 on planes where every (or every other) 32x32 block is wide: the
    int8 fix-up launch (a small grid walking the blocks, k_tc32_mfma<.., FIXUP>)
    must code each marked block -- thousands per plane, many per wave -- exactly
    as the int8-only launch (variant 2) does; the oracle checks a corner."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(77)
    nf, w, h = 2, 3840, 2160
    sets = gpu.yuv420_plane_sets(nf, w, h)
    fe = gpu.yuv420_frame_elems(w, h)
    buf = rng.integers(0, 256, size=nf * fe).astype(np.int16)
    buf[:w * h] = rng.integers(-32768, 32768, size=w * h)          # frame 0 luma: every block wide
    cb = buf[fe:fe + w * h].reshape(h, w)
    cb[::64, ::64] = 999                                            # frame 1 luma: every other block row/col wide
    d = torch.from_numpy(buf).cuda()
    outs = []
    for v in (1, 2):
        lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
        rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
        gpu.tc32_planes(d, sets, 30, v, lvl=lvl, rec=rec)
        outs.append((lvl, rec))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    corner = buf[:w * h].reshape(h, w)[:64, :96]
    el, er = O.tc32_plane(corner.copy(), 30)
    got = outs[0][1][:w * h].view(h, w)[:64, :96].cpu().numpy()
    assert np.array_equal(got, er)


@pytest.mark.parametrize("variant", [1, 2, 0])
def test_tc32_planes_stream_equals_per_plane_and_oracle(nh, torch_dev, variant):
    """Config 5 batched over a ragged YUV420 frame stream (one MFMA launch per
    plane set) == the per-plane entry point == the oracle, every plane."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(55)
    nf, w, h = 3, 208, 136                         # partial 32x32 blocks in every plane (pitches % 8 == 0)
    sets = gpu.yuv420_plane_sets(nf, w, h)
    fe = gpu.yuv420_frame_elems(w, h)
    buf = rng.integers(0, 256, size=nf * fe).astype(np.int16)
    buf[fe:2 * fe] = rng.integers(-32768, 32768, size=fe)   # frame 1: int16 extremes (3-part split)
    buf[2 * fe + 5 * w + 40] = 300                          # frame 2: one wide block among 8-bit ones
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(d.shape, -7, dtype=torch.int32, device="cuda")   # untouched outside full blocks
    rec = torch.full(d.shape, -7, dtype=torch.int16, device="cuda")
    gpu.tc32_planes(d, sets, 30, variant, lvl=lvl, rec=rec)
    lv, rv = lvl.cpu().numpy(), rec.cpu().numpy()
    for f in range(nf):
        off = f * fe
        for (ph, pw) in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er = O.tc32_plane(src, 30)
            pl, pr = gpu.tc32_plane(torch.from_numpy(src.copy()).cuda(), 30, variant)
            got_l, got_r = lv[off:off + ph * pw].reshape(ph, pw), rv[off:off + ph * pw].reshape(ph, pw)
            fh, fw = ph // 32 * 32, pw // 32 * 32
            assert np.array_equal(got_l[:fh, :fw], el[:fh, :fw]) and np.array_equal(got_r[:fh, :fw], er[:fh, :fw]), (f, ph)
            assert np.array_equal(got_l[:fh, :fw], pl.cpu().numpy()[:fh, :fw]), (f, ph)
            assert (got_l[fh:, :] == -7).all() and (got_l[:, fw:] == -7).all(), (f, ph)
            off += ph * pw


def test_tu_pipeline_int16_extremes(nh, torch_dev):
    """Config 4 on arbitrary int16 samples: the 24-bit mad bounds hold at every TU size."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(31)
    src = rng.integers(-32768, 32768, size=(96, 128)).astype(np.int16)
    for luma, ctb in ((True, 32), (False, 16)):
        l, r, t = gpu.tu_pipeline_plane(torch.from_numpy(src).cuda(), ctb, int(not luma), 5, 3, luma)
        el, er, et = O.tu_pipeline_plane(src, ctb, int(not luma), 5, 3, luma)
        assert np.array_equal(l.cpu().numpy(), el) and np.array_equal(r.cpu().numpy(), er)


@pytest.mark.parametrize("qp", [0, 22, 51])
def test_tu_pipeline_narrow_extremes_and_mixed(nh, torch_dev, qp):
    """Config 4's packed 16-bit chain (narrow workgroups) at its
    range limits -- samples only 0 / 255, so residuals reach +-255 -- and planes
    where a few samples leave [0, 255] (those workgroups take the 32-bit chain,
    their neighbours the packed one), against the oracle at QP 0 / 22 / 51."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(90 + qp)
    h, w = 200, 264
    two = (rng.integers(0, 2, size=(h, w)) * 255).astype(np.int16)
    mixed = np.clip(128 + rng.integers(-60, 61, size=(h, w)), 0, 255).astype(np.int16)
    for y, x, v in ((5, 7, 256), (70, 130, -1), (150, 40, 4000), (199, 263, -300), (31, 100, 511)):
        mixed[y, x] = v
    for src in (two, mixed):
        for luma, ctb in ((True, 32), (False, 16)):
            l, r, t = gpu.tu_pipeline_plane(torch.from_numpy(src).cuda(), ctb, int(not luma), 13, qp, luma)
            el, er, et = O.tu_pipeline_plane(src, ctb, int(not luma), 13, qp, luma)
            assert np.array_equal(t.cpu().numpy(), et)
            assert np.array_equal(l.cpu().numpy(), el), (luma, qp)
            assert np.array_equal(r.cpu().numpy(), er), (luma, qp)


# ------------------------------------------------------------------ f-4: fused level-side epilogue

def _ref_level_helpers(lv, sets):
    """count_nonzero / estimate_bits (quant.py:153-173) of every full 8x8 block,
    in the launch's block order, with the reference's own numpy formula."""
    nnz, bits = [], []
    for s in sets:
        for g in range(s.num_groups):
            for c in range(s.planes_per_group):
                o = s.base + g * s.group_stride + c * s.plane_stride
                p = lv[o:o + s.height * s.pitch].reshape(s.height, s.pitch)[:s.height // 8 * 8, :s.width // 8 * 8]
                blk = p.reshape(s.height // 8, 8, s.width // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
                a = np.abs(blk.astype(np.int32))
                nnz.append(np.count_nonzero(blk, axis=1))
                bits.append(np.sum(np.log2(a + 1) + (a > 0) * 2, axis=1).astype(np.int64))   # int() of a float >= 0
    return np.concatenate(nnz), np.concatenate(bits)


@pytest.mark.parametrize("qp,intra,kind", [(32, True, "noise"), (4, True, "noise"), (22, False, "natural"),
                                           (0, True, "int16")])
def test_fused8x8_epilogue_vs_reference_helpers(nh, torch_dev, qp, intra, kind):
    torch = torch_dev
    from nano_hevc import gpu, quant
    F, W, H = 2, 352, 288
    fe = gpu.yuv420_frame_elems(W, H)
    rng = np.random.default_rng(qp + 7)
    if kind == "int16":
        buf = rng.integers(-32768, 32768, size=F * fe).astype(np.int16)
    elif kind == "noise":
        buf = rng.integers(-255, 256, size=F * fe).astype(np.int16)
    else:
        planes = []
        for f in range(F):
            for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
                yy, xx = np.mgrid[0:ph, 0:pw]
                planes.append(natural_residual(np.clip(60 + (2 * xx + yy + f) % 150 + rng.integers(-9, 10, (ph, pw)),
                                                       0, 255)).reshape(-1))
        buf = np.concatenate(planes)
    d = torch.from_numpy(buf).cuda()
    sets = gpu.yuv420_plane_sets(F, W, H)
    lv, nnz, bits = gpu.fwd8x8_quant_ex(d, sets, qp, intra)
    lv = lv.cpu().numpy()
    assert np.array_equal(lv, gpu.fwd8x8_quant(d, sets, qp, intra).cpu().numpy())
    enz, ebits = _ref_level_helpers(lv, sets)
    assert np.array_equal(nnz.cpu().numpy(), enz)
    assert np.array_equal(bits.cpu().numpy(), ebits)
    # spot-check the vectorised expectation against the drop-in per-block helpers
    blk = lv[:8 * W].reshape(8, W)[:, :64].reshape(8, 8, 8).transpose(1, 0, 2)
    for k in range(8):
        b32 = blk[k].astype(np.int32)
        assert quant.count_nonzero(b32) == enz[k] and quant.estimate_bits(b32) == ebits[k]
    # optional outputs
    _, n2, b2 = gpu.fwd8x8_quant_ex(d, sets, qp, intra, bits=False)
    assert b2 is None and torch.equal(n2, nnz)


# ------------------------------------------------------------------ f-1: closed-loop config 3 (wavefront)

@pytest.mark.parametrize("key", ["c3a", "c3b", "c3c"])
def test_intra_rdo_closed_golden(nh, torch_dev, golden, key):
    """Closed loop vs planes composed from the reference's own BlockView /
    Plane / predictor / transform / quant functions (make_golden.gen_closed)."""
    torch = torch_dev
    from nano_hevc import gpu
    g = golden("closed.npz")
    src = g[key + "_src"]
    h, w = src.shape
    d = torch.from_numpy(src.reshape(-1).copy()).cuda()
    modes, lvl, rec, sse = gpu.intra_rdo_closed(d, [gpu.plane_set(0, w, h, w)], int(g[key + "_qp"]))
    assert np.array_equal(modes.cpu().numpy().reshape(h // 8, w // 8), g[key + "_modes"])
    assert np.array_equal(lvl.cpu().numpy().reshape(h, w), g[key + "_lvl"])
    assert np.array_equal(rec.cpu().numpy().reshape(h, w), g[key + "_rec"])
    assert int(sse.cpu()[0]) == int(g[key + "_sse"])


@pytest.mark.parametrize("F,W,H,qp", [(4, 352, 288, 32), (2, 200, 104, 22)])
def test_intra_rdo_closed_stream_vs_oracle(nh, torch_dev, F, W, H, qp):
    """Many planes at once (concurrent wavefronts, rows of different planes
    interleaved by the ticket order): every plane equals the sequential oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(F * 1000 + qp)
    planes = []
    for f in range(F):
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            planes.append(np.clip(50 + (2 * xx + 3 * yy + 11 * f) % 160 + rng.integers(-10, 11, (ph, pw)), 0, 255)
                          .astype(np.int16))
    buf = np.concatenate([p.reshape(-1) for p in planes])
    d = torch.from_numpy(buf).cuda()
    sets = gpu.yuv420_plane_sets(F, W, H)
    modes, lvl, rec, sse = gpu.intra_rdo_closed(d, sets, qp)
    modes, lvl, rec, sse = modes.cpu().numpy(), lvl.cpu().numpy(), rec.cpu().numpy(), sse.cpu().numpy()
    # plane order of the outputs: all Y planes (set 0), then U, V of each frame (set 1)
    order = [3 * f for f in range(F)] + [3 * f + c for f in range(F) for c in (1, 2)]
    offs = np.cumsum([0] + [p.size for p in planes])
    m0 = 0
    for k, pi in enumerate(order):
        p = planes[pi]
        ph, pw = p.shape
        em, el, er, es = O.intra_rdo_plane(p, qp, closed=True)
        n = (ph // 8) * (pw // 8)
        assert np.array_equal(modes[m0:m0 + n].reshape(ph // 8, pw // 8), em), (k, pi)
        m0 += n
        o = offs[pi]
        assert np.array_equal(lvl[o:o + p.size].reshape(p.shape), el), (k, pi)
        assert np.array_equal(rec[o:o + p.size].reshape(p.shape), er), (k, pi)
        assert int(sse[k]) == es
    # the closed loop is a different encoder than the open loop
    _, _, ro, _ = O.intra_rdo_plane(planes[0], qp)
    assert not np.array_equal(ro, rec[:planes[0].size].reshape(planes[0].shape))


@pytest.mark.parametrize("batch,depth,pad", [(3, 2, 0), (2, 3, 16), (1, 4, 0), (9, 3, 8)])
def test_intra_rdo_closed_batches_equal_one_call(nh, torch_dev, batch, depth, pad):
    """intra_rdo_closed_yuv420_stream: a 7-frame stream in batches over rotating
    streams (a ragged last batch, a padded frame stride, a base offset, one frame
    with a 9-bit sample: its batch alone takes the 32-bit form) gives the outputs,
    in the same layout, of one intra_rdo_closed call; frame 0's Y plane equals
    the oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H, qp, base = 7, 72, 48, 27, 24
    rng = np.random.default_rng(900 + batch * 10 + depth)
    fe = gpu.yuv420_frame_elems(W, H)
    fs = fe + pad
    buf = np.zeros(base + F * fs, np.int16)
    for f in range(F):
        off = base + f * fs
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = np.clip(50 + (2 * xx + 3 * yy + 11 * f) % 160 + rng.integers(-20, 21, (ph, pw)), 0, 255)
            if f == 5:
                p[ph // 3, pw // 2] = 300
            buf[off:off + ph * pw] = p.reshape(-1)
            off += ph * pw
    d = torch.from_numpy(buf).cuda()
    m1, l1, r1, s1 = gpu.intra_rdo_closed_yuv420_stream(d, W, H, F, qp, batch_frames=batch, depth=depth,
                                                        frame_stride=fs, base=base)
    m0, l0, r0, s0 = gpu.intra_rdo_closed(d, gpu.yuv420_plane_sets(F, W, H, fs, base), qp)
    assert torch.equal(m1, m0) and torch.equal(l1, l0) and torch.equal(r1, r0) and torch.equal(s1, s0)
    y0 = buf[base:base + W * H].reshape(H, W)
    em, el, er, es = O.intra_rdo_plane(y0, qp, closed=True)
    assert np.array_equal(m1[:(H // 8) * (W // 8)].cpu().numpy().reshape(H // 8, W // 8), em)
    assert np.array_equal(r1[base:base + W * H].cpu().numpy().reshape(H, W), er) and int(s1[0]) == es


def test_intra_rdo_closed_ragged_and_int16(nh, torch_dev):
    """Partial blocks (recon 0 there, and read as 0 by the top-right references)
    and full-range int16 sources."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(55)
    for src, qp in ((rng.integers(0, 256, (45, 67)).astype(np.int16), 27),
                    (rng.integers(-32768, 32768, (24, 40)).astype(np.int16), 12)):
        h, w = src.shape
        d = torch.from_numpy(src.reshape(-1).copy()).cuda()
        rec_in = torch.full((h * w,), 777, dtype=torch.int16, device="cuda")
        modes, lvl, rec, sse = gpu.intra_rdo_closed(d, [gpu.plane_set(0, w, h, w)], qp, rec=rec_in)
        em, el, er, es = O.intra_rdo_plane(src, qp, closed=True)
        assert np.array_equal(modes.cpu().numpy().reshape(h // 8, w // 8), em)
        assert np.array_equal(rec.cpu().numpy().reshape(h, w), er)
        assert np.array_equal(lvl.cpu().numpy().reshape(h, w)[:h // 8 * 8, :w // 8 * 8], el[:h // 8 * 8, :w // 8 * 8])
        assert int(sse.cpu()[0]) == es


@pytest.mark.parametrize("variant", [17, 21, 9, 13, 33, 97, 32, 35, 129, 128, 261, 517, 773, 257, 2052, 2053, 4096 + 5, 4096 + 16 * 3 + 5, 4096 + 16 * 15 + 5, 8192 + 33, 8192 + 97, 16384 + 1, 16384, 4096 + 16 * 15 + 9, 32768 + 8, 32768 + 1])
def test_fused8x8_launch_variants_equal(nh, torch_dev, variant):
    """Every A/B launch form (pipelined 9/13, vertical block pair 17/21, stripe
    form by LDS-DMA 33/32/35, register-staged 97, persistent double-buffered 129/128) gives
    the default kernel's levels: a 4K YUV420 stream (135 chroma block rows: pairs
    straddle planes) and ragged planes with an odd number of block rows."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(variant)
    F, W, H = 3, 3840, 2160
    fe = gpu.yuv420_frame_elems(W, H)
    buf = torch.from_numpy(rng.integers(-32768, 32768, size=F * fe).astype(np.int16)).cuda()
    sets = gpu.yuv420_plane_sets(F, W, H)
    ref = gpu.fwd8x8_quant(buf, sets, 27, True)
    assert torch.equal(gpu.fwd8x8_quant(buf, sets, 27, True, variant=variant), ref)
    plane = rng.integers(-255, 256, size=(3 * 40 * 56,)).astype(np.int16)   # 3 planes of 40x56: 5 block rows each
    d = torch.from_numpy(plane).cuda()
    s1 = [gpu.plane_set(0, 56, 40, 56, 1, 3, 0, 40 * 56)]
    out = gpu.fwd8x8_quant(d, s1, 32, False, variant=variant).cpu().numpy()
    for k in range(3):
        p = plane[k * 2240:(k + 1) * 2240].reshape(40, 56)
        assert np.array_equal(out[k * 2240:(k + 1) * 2240].reshape(40, 56), O.fwd8x8_quant_plane(p, 32, False))


@pytest.mark.parametrize("W,H,rows", [(640, 360, (0, 1 << 30)), (200, 120, (1, 3))])
def test_tu_pipeline_planes_batched_vs_oracle(nh, torch_dev, W, H, rows):
    """Config 4 over a whole YUV420 stream in one launch per TU size and plane
    set (luma set: ctb 32, plane id 0; U+V set: ctb 16, ids 1/2): every plane
    equals the per-plane oracle (also on a CTU-row band)."""
    torch = torch_dev
    from nano_hevc import gpu
    F = 3
    rng = np.random.default_rng(W + F)
    planes = []
    for f in range(F):
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            planes.append(np.clip(70 + (xx + 2 * yy + 9 * f) % 140 + rng.integers(-20, 21, (ph, pw)), 0, 255).astype(np.int16))
    buf = np.concatenate([p.reshape(-1) for p in planes])
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
    _, _, tuy = gpu.tu_pipeline_planes(d, sy, 32, 0, 4242, 30, True, *rows, lvl=lvl, rec=rec)
    _, _, tuc = gpu.tu_pipeline_planes(d, suv, 16, 1, 4242, 30, False, *rows, lvl=lvl, rec=rec)
    lvl, rec, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    offs = np.cumsum([0] + [p.size for p in planes])
    for k, p in enumerate(planes):
        f, c = divmod(k, 3)
        el, er, et = O.tu_pipeline_plane(p, 32 if c == 0 else 16, c, 4242, 30, c == 0, *rows)
        o = offs[k]
        assert np.array_equal(lvl[o:o + p.size].reshape(p.shape), el), (f, c)
        assert np.array_equal(rec[o:o + p.size].reshape(p.shape), er), (f, c)
        assert np.array_equal(tuy[f] if c == 0 else tuc[2 * f + c - 1], et), (f, c)


@pytest.mark.parametrize("layout", ["pitch+2", "base+2"])
@pytest.mark.parametrize("qp", [0, 22, 51])
def test_tu_pipeline_layout_fallback_vs_oracle(nh, torch_dev, layout, qp):
    """Layouts the CTU-granular kernel's vector accesses cannot take -- a pitch
    that is not a multiple of 4 elements, or a plane base 2 elements off (source
    / recon rows not 8-B aligned, level rows not 16-B aligned) -- make
    ctu_open_launch return NH_EVALUE and nh_tu_pipeline_planes fall back to the
    per-size launches (k_tu_process, 32x32 TUs on the butterfly).  That path
    against the oracle: luma (CTB 32) and chroma (CTB 16), 8-bit and int16
    content, two planes per set (group stride), partial CTUs."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(17 + qp)
    W, H = 200, 136
    pitch, base = (W + 2, 0) if layout == "pitch+2" else (W, 2)
    gs = pitch * H + 6
    eight = [np.clip(120 + rng.integers(-70, 71, (H, W)), 0, 255).astype(np.int16) for _ in range(2)]
    wide = [rng.integers(-32768, 32768, (H, W)).astype(np.int16) for _ in range(2)]
    for planes in (eight, wide):
        buf = np.zeros(base + 2 * gs, np.int16)
        for g, p in enumerate(planes):
            for y in range(H):
                o = base + g * gs + y * pitch
                buf[o:o + W] = p[y]
        d = torch.from_numpy(buf).cuda()
        for luma, ctb, pid in ((True, 32, 0), (False, 16, 1)):
            lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
            rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
            pset = gpu.plane_set(base, W, H, pitch, 1, 2, 0, gs)
            _, _, tu = gpu.tu_pipeline_planes(d, pset, ctb, pid, 77, qp, luma, lvl=lvl, rec=rec)
            lv, rc, tu = lvl.cpu().numpy(), rec.cpu().numpy(), tu.cpu().numpy()
            for g, p in enumerate(planes):
                el, er, et = O.tu_pipeline_plane(p, ctb, pid, 77, qp, luma)
                rows = [slice(base + g * gs + y * pitch, base + g * gs + y * pitch + W) for y in range(H)]
                assert np.array_equal(np.stack([lv[r] for r in rows]), el), (layout, luma, g)
                assert np.array_equal(np.stack([rc[r] for r in rows]), er), (layout, luma, g)
                assert np.array_equal(tu[g], et), (layout, luma, g)


def test_fused8x8_stripe_form_needs_contiguous_rows(nh, torch_dev):
    """The stripe form (variant 33) walks a tile as one contiguous range: a plane
    whose pitch is not 8 * (width // 8) is refused, never silently mis-read."""
    torch = torch_dev
    from nano_hevc import gpu
    d = torch.zeros(64 * 72, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError, match="stripe form"):
        gpu.fwd8x8_quant(d, [gpu.plane_set(0, 60, 64, 72)], 32, True, variant=33)


@pytest.mark.parametrize("key", ["k4y", "k4u", "k4n", "k4r"])
def test_tu_pipeline_closed_golden(nh, torch_dev, golden, key):
    """Closed-loop config 4 vs planes composed from the reference's own
    BlockView / Plane / predictors / chain (make_golden.gen_closed4)."""
    torch = torch_dev
    from nano_hevc import gpu
    g = golden("closed4.npz")
    src = g[key + "_src"]
    h, w = src.shape
    hh, ww = h // 4 * 4, w // 4 * 4          # the device path takes w, h multiples of 4
    d = torch.from_numpy(np.ascontiguousarray(src[:hh, :ww]).reshape(-1)).cuda()
    lvl, rec, tu = gpu.tu_pipeline_closed(d, gpu.plane_set(0, ww, hh, ww), int(g[key + "_ctb"]), int(g[key + "_pid"]),
                                          1234, int(g[key + "_qp"]), bool(g[key + "_luma"]))
    lvl, rec = lvl.cpu().numpy().reshape(hh, ww), rec.cpu().numpy().reshape(hh, ww)
    if (hh, ww) == (h, w):
        assert np.array_equal(lvl, g[key + "_lvl"]) and np.array_equal(rec, g[key + "_rec"])
        assert np.array_equal(tu.cpu().numpy()[0], g[key + "_tu"])
    else:   # ragged plane: the oracle on the multiple-of-4 crop (the fixture pins the oracle itself)
        el, er, et = O.tu_pipeline_plane_closed(np.ascontiguousarray(src[:hh, :ww]), int(g[key + "_ctb"]),
                                                int(g[key + "_pid"]), 1234, int(g[key + "_qp"]), bool(g[key + "_luma"]))
        assert np.array_equal(lvl, el) and np.array_equal(rec, er) and np.array_equal(tu.cpu().numpy()[0], et)


@pytest.mark.parametrize("conc", [False, True])
@pytest.mark.parametrize("F,W,H,qp", [(3, 104, 72, 32), (2, 136, 104, 12)])
def test_tu_pipeline_closed_stream_vs_oracle(nh, torch_dev, F, W, H, qp, conc):
    """A YUV420 frame stream in two launches (luma CTB 32, chroma CTB 16, plane
    ids 0 / 1, 2), in sequence or as concurrent wavefronts on two streams
    (tu_pipeline_closed_yuv420): many CTU wavefronts at once, partial CTUs,
    8-bit content and an int16-extreme frame; every plane equals the
    sequential oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(F * 100 + qp)
    fe = gpu.yuv420_frame_elems(W, H)
    buf = np.empty(F * fe, np.int16)
    off = 0
    for f in range(F):
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = np.clip(60 + (3 * xx + 2 * yy + 7 * f) % 150 + rng.integers(-12, 13, (ph, pw)), 0, 255)
            if f == 1:
                p = rng.integers(-32768, 32768, (ph, pw))
            buf[off:off + ph * pw] = p.reshape(-1)
            off += ph * pw
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
    if conc:
        _, _, tuy, tuc = gpu.tu_pipeline_closed_yuv420(d, sy, suv, 777, qp, lvl=lvl, rec=rec)
    else:
        _, _, tuy = gpu.tu_pipeline_closed(d, sy, 32, 0, 777, qp, True, lvl=lvl, rec=rec)
        _, _, tuc = gpu.tu_pipeline_closed(d, suv, 16, 1, 777, qp, False, lvl=lvl, rec=rec)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    off = 0
    for f in range(F):
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 777, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw


@pytest.mark.parametrize("batch,depth,pad", [(3, 2, 0), (3, 3, 0), (2, 4, 24), (1, 3, 8), (8, 3, 0)])
def test_tu_pipeline_closed_batches_vs_oracle(nh, torch_dev, batch, depth, pad):
    """tu_pipeline_closed_yuv420_stream: a 7-frame YUV420 stream in batches of
    ``batch`` frames over ``depth`` stream pairs (batches in flight together, a
    ragged last batch, a frame stride with ``pad`` spare samples and a base
    offset), one 9-bit frame (its batch alone takes the 32-bit form); every
    plane equals the sequential oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H, qp, base = 7, 136, 104, 27, 40
    rng = np.random.default_rng(7000 + batch * 10 + depth)
    fe = gpu.yuv420_frame_elems(W, H)
    fs = fe + pad
    buf = np.zeros(base + F * fs, np.int16)
    for f in range(F):
        off = base + f * fs
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = np.clip(60 + (3 * xx + 2 * yy + 13 * f) % 150 + rng.integers(-25, 26, (ph, pw)), 0, 255)
            if f == 4:
                p[ph // 2, pw // 3] = 300
            buf[off:off + ph * pw] = p.reshape(-1)
            off += ph * pw
    d = torch.from_numpy(buf).cuda()
    lvl, rec, tuy, tuc = gpu.tu_pipeline_closed_yuv420_stream(d, W, H, F, 555, qp, batch_frames=batch, depth=depth,
                                                              frame_stride=fs, base=base)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    assert tuy.shape == (F, H // 4, W // 4) and tuc.shape == (2 * F, H // 8, W // 8)
    for f in range(F):
        off = base + f * fs
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 555, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw
        assert not lv[off:base + (f + 1) * fs].any() and not rv[off:base + (f + 1) * fs].any()   # the pad untouched


@pytest.mark.parametrize("conc", [False, True])
@pytest.mark.parametrize("F,W,H,qp", [(1, 104, 72, 32), (2, 136, 104, 22), (3, 104, 72, 32), (5, 72, 40, 0), (2, 136, 104, 4),
                                      (4, 136, 104, 51)])
def test_tu_pipeline_closed_pairs_vs_oracle(nh, torch_dev, F, W, H, qp, conc):
    """8-bit YUV420 streams in closed loop: the plane-pair form (one wave codes
    the same CTU row of frames 2p and 2p + 1, their TUs in shared batches) for
    even and odd frame counts (a lone last plane), partial CTUs, QP 0 / 51 and
    0 / 255 extremes; every plane equals the sequential oracle."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(F * 1000 + W + qp)
    fe = gpu.yuv420_frame_elems(W, H)
    buf = np.empty(F * fe, np.int16)
    off = 0
    for f in range(F):
        for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            if f == 2:   # residuals at the extremes of the 8-bit range
                p = 255 * rng.integers(0, 2, (ph, pw))
            else:
                p = np.clip(60 + (3 * xx + 2 * yy + 11 * f) % 150 + rng.integers(-30, 31, (ph, pw)), 0, 255)
            buf[off:off + ph * pw] = p.reshape(-1)
            off += ph * pw
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
    if conc:
        _, _, tuy, tuc = gpu.tu_pipeline_closed_yuv420(d, sy, suv, 4242, qp, lvl=lvl, rec=rec)
    else:
        _, _, tuy = gpu.tu_pipeline_closed(d, sy, 32, 0, 4242, qp, True, lvl=lvl, rec=rec)
        _, _, tuc = gpu.tu_pipeline_closed(d, suv, 16, 1, 4242, qp, False, lvl=lvl, rec=rec)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    off = 0
    for f in range(F):
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 4242, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw


@pytest.mark.parametrize("where,F", [("last", 4), ("first", 4), ("chroma_v_last", 3), ("chroma_u_neg", 3),
                                     ("luma_lone_last", 3)])
def test_tu_pipeline_closed_pairs_late_wide_sample(nh, torch_dev, where, F):
    """The pair kernel checks the source samples its chains load (round 5; no scan
    before the launch): ONE 9-bit sample in the last CTU of the last frame's luma --
    found after every other row is coded -- or in the first CTU of the first frame
    sends the whole set to the 32-bit form behind it (its own tickets and line-word
    tags); every plane equals the sequential oracle.  Also the chroma instance (4
    planes per wave; F = 3: the last group holds 2 planes) with the wide sample only
    in the last V plane or a negative one in a U plane, and a lone last luma plane
    (F = 3: npl = 1) holding it."""
    torch = torch_dev
    from nano_hevc import gpu
    W, H, qp = 104, 72, 27
    rng = np.random.default_rng(404)
    fe = gpu.yuv420_frame_elems(W, H)
    cw, ch = W // 2, H // 2
    buf = np.clip(100 + rng.integers(-90, 91, F * fe), 0, 255).astype(np.int16)
    if where in ("last", "luma_lone_last"):
        buf[(F - 1) * fe + (H - 3) * W + W - 5] = 300   # inside the bottom-right whole CTU's TUs
    elif where == "first":
        buf[7 * W + 3] = -4
    elif where == "chroma_v_last":                      # the last frame's V plane, bottom-right CTU
        buf[(F - 1) * fe + W * H + cw * ch + (ch - 2) * cw + cw - 3] = 511
    else:                                               # frame 1's U plane, an inner CTU
        buf[fe + W * H + 20 * cw + 21] = -1
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
    _, _, tuy, tuc = gpu.tu_pipeline_closed_yuv420(d, sy, suv, 31, qp, lvl=lvl, rec=rec)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    for f in range(F):
        off = f * fe
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 31, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw


def test_tu_pipeline_closed_pairs_many_frames_vs_oracle(nh, torch_dev):
    """2048 small 8-bit YUV420 frames (72x40: whole and ragged CTUs) in one
    concurrent launch pair: >= 4096 CTU rows per launch, so whole CTUs leave
    their packed-chain recon from the LDS reconstruction at the CTU's end
    (Closed4Args::rec_ctu) and ragged ones per TU; sampled frames equal the
    sequential oracle and untouched-by-TU samples stay zero."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H, qp = 2048, 72, 40, 27
    rng = np.random.default_rng(2048)
    fe = gpu.yuv420_frame_elems(W, H)
    buf = np.clip(90 + rng.integers(-80, 81, F * fe), 0, 255).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
    _, _, tuy, tuc = gpu.tu_pipeline_closed_yuv420(d, sy, suv, 99, qp, lvl=lvl, rec=rec)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    for f in (0, 1, 1023, 2047):
        off = f * fe
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 99, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw


@pytest.mark.parametrize("lead", [1, 2])
def test_tu_pipeline_closed_pairs_offset_planes_vs_oracle(nh, torch_dev, lead):
    """The pair form with the plane sets starting `lead` samples into the buffer:
    lead 1 (odd base: 2-B aligned rows) and lead 2 (4-B aligned) both take the
    packed 32x32 chain (the f16 matrix-core chain needs 16-B level rows); both
    equal the oracle, and the leading samples stay untouched."""
    torch = torch_dev
    from nano_hevc import gpu
    F, W, H, qp = 3, 104, 72, 30
    rng = np.random.default_rng(lead)
    fe = gpu.yuv420_frame_elems(W, H)
    buf = np.clip(70 + rng.integers(-60, 61, lead + F * fe), 0, 255).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    sy, suv = gpu.yuv420_plane_sets(F, W, H, base=lead)
    lvl = torch.full(d.shape, -9, dtype=torch.int32, device="cuda")
    rec = torch.full(d.shape, -9, dtype=torch.int16, device="cuda")
    _, _, tuy, tuc = gpu.tu_pipeline_closed_yuv420(d, sy, suv, 777, qp, lvl=lvl, rec=rec)
    lv, rv, tuy, tuc = lvl.cpu().numpy(), rec.cpu().numpy(), tuy.cpu().numpy(), tuc.cpu().numpy()
    assert (lv[:lead] == -9).all() and (rv[:lead] == -9).all()
    off = lead
    for f in range(F):
        for k, (pw, ph) in enumerate(((W, H), (W // 2, H // 2), (W // 2, H // 2))):
            src = buf[off:off + ph * pw].reshape(ph, pw)
            el, er, et = O.tu_pipeline_plane_closed(src, 32 if k == 0 else 16, k, 777, qp, k == 0)
            assert np.array_equal(lv[off:off + ph * pw].reshape(ph, pw), el), (f, k)
            assert np.array_equal(rv[off:off + ph * pw].reshape(ph, pw), er), (f, k)
            assert np.array_equal(tuy[f] if k == 0 else tuc[2 * f + k - 1], et), (f, k)
            off += ph * pw


@pytest.mark.parametrize("ctb", [4, 8, 16])
def test_tu_pipeline_closed_small_ctb_vs_oracle(nh, torch_dev, ctb):
    """Closed-loop config 4 with CTBs below 32 (fewer units per CTU, more CTU rows)."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(ctb)
    h, w = 44, 60
    src = np.clip(90 + rng.integers(-40, 41, (h, w)), 0, 255).astype(np.int16)
    d = torch.from_numpy(src.reshape(-1).copy()).cuda()
    lvl, rec, tu = gpu.tu_pipeline_closed(d, gpu.plane_set(0, w, h, w), ctb, 0, 99, 27, True)
    el, er, et = O.tu_pipeline_plane_closed(src, ctb, 0, 99, 27, True)
    assert np.array_equal(lvl.cpu().numpy().reshape(h, w), el)
    assert np.array_equal(rec.cpu().numpy().reshape(h, w), er)
    assert np.array_equal(tu.cpu().numpy()[0], et)


@pytest.mark.parametrize("ldt", ["int16", "int8"])
def test_tc32_compact_levels_equal_int32_path(nh, torch_dev, ldt):
    """Config 5 with compact levels (k_tc32_hd<2, int16 / int8>) over a ragged
    YUV420 stream with wide frames: every 8-bit block's compact level equals the
    int32 path's, every wide block carries the spill marker at its origin with its
    int32 levels in the spill plane, and the widened levels equal tc32_planes' (and
    the oracle's) everywhere; recon identical; outside full blocks untouched."""
    torch = torch_dev
    from nano_hevc import gpu
    dt = getattr(torch, ldt)
    rng = np.random.default_rng(66)
    nf, w, h = 3, 224, 136                       # chroma pitch 112: 16-element aligned (int8 rows)
    sets = gpu.yuv420_plane_sets(nf, w, h)
    fe = gpu.yuv420_frame_elems(w, h)
    buf = rng.integers(0, 256, size=nf * fe).astype(np.int16)
    buf[fe:2 * fe] = rng.integers(-32768, 32768, size=fe)   # frame 1: every block wide
    buf[2 * fe + 5 * w + 40] = 300                          # frame 2: one wide luma block
    buf[2 * fe + w * h + 3 * (w // 2) + 70] = -1            # ... and one wide U block
    d = torch.from_numpy(buf).cuda()
    for qp in (0, 4, 30, 51):
        lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
        rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
        gpu.tc32_planes(d, sets, qp, 1, lvl=lvl, rec=rec)
        lc = torch.full(d.shape, 5, dtype=dt, device="cuda")
        rc = torch.full(d.shape, -7, dtype=torch.int16, device="cuda")
        lc, rc, spill = gpu.tc32_planes_compact(d, sets, qp, dt, lvl=lc, rec=rc)
        out = torch.full(d.shape, -9, dtype=torch.int32, device="cuda")
        wide = gpu.tc32_levels_widen(lc, spill, sets, out=out)
        lv, rv, cv, wv, wr = (lvl.cpu().numpy(), rec.cpu().numpy(), lc.cpu().numpy(), wide.cpu().numpy(),
                              rc.cpu().numpy())
        mark = -32768 if ldt == "int16" else -128
        for f in range(nf):
            off = f * fe
            for (ph, pw) in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
                fh, fw = ph // 32 * 32, pw // 32 * 32
                src = buf[off:off + ph * pw].reshape(ph, pw)
                L, R = lv[off:off + ph * pw].reshape(ph, pw), rv[off:off + ph * pw].reshape(ph, pw)
                Cc, Wd = cv[off:off + ph * pw].reshape(ph, pw), wv[off:off + ph * pw].reshape(ph, pw)
                Rc = wr[off:off + ph * pw].reshape(ph, pw)
                assert np.array_equal(Wd[:fh, :fw], L[:fh, :fw]), (qp, f, ph)
                assert np.array_equal(Rc[:fh, :fw], R[:fh, :fw]), (qp, f, ph)
                assert (Wd[fh:, :] == -9).all() and (Wd[:, fw:] == -9).all()
                assert (Cc[fh:, :] == 5).all() and (Cc[:, fw:] == 5).all()
                for by in range(0, fh, 32):
                    for bx in range(0, fw, 32):
                        parts = [src[by:by + 32, bx:bx + 32].ravel()]   # the block, the row above, the column left
                        if by:
                            parts.append(src[by - 1, bx:bx + 32])
                        if bx:
                            parts.append(src[by:by + 32, bx - 1])
                        blk = np.concatenate(parts)
                        narrow = blk.min() >= 0 and blk.max() <= 255
                        if narrow:
                            assert np.array_equal(Cc[by:by + 32, bx:bx + 32], L[by:by + 32, bx:bx + 32]), (qp, f, by, bx)
                            assert np.abs(L[by:by + 32, bx:bx + 32]).max() <= 51
                        else:
                            assert Cc[by, bx] == mark, (qp, f, by, bx)
                if f == 2 and ph == h:
                    el, er = O.tc32_plane(src, qp)
                    assert np.array_equal(Wd[:fh, :fw], el[:fh, :fw]) and np.array_equal(Rc[:fh, :fw], er[:fh, :fw])
                off += ph * pw


def test_tc32_compact_levels_refuse_bad_layouts(nh, torch_dev):
    """int8 levels need 16-element aligned rows and planes; only variant 1 has
    compact levels (tc32_planes keeps int32)."""
    torch = torch_dev
    from nano_hevc import gpu
    d = torch.zeros(3 * gpu.yuv420_frame_elems(208, 136), dtype=torch.int16, device="cuda")
    sets = gpu.yuv420_plane_sets(3, 208, 136)     # chroma pitch 104: 8- but not 16-element aligned
    with pytest.raises(ValueError):
        gpu.tc32_planes_compact(d, sets, 30, torch.int8)
    gpu.tc32_planes_compact(d, sets, 30, torch.int16)
    with pytest.raises(TypeError):
        gpu.tc32_planes_compact(d, sets, 30, torch.int32)


@pytest.mark.parametrize("qp", [0, 22, 51])
def test_tu_compact_levels_equal_int32_path(nh, torch_dev, qp):
    """Config 4 with compact int16 levels over a ragged YUV420 stream with a wide
    frame (int16 extremes: every group on the 32-bit chain) and a frame with one
    9-bit luma sample and one negative chroma sample (one wide group each among 8-bit
    ones): the widened levels, recon and TU maps equal tu_pipeline_planes' (int32);
    every 8-bit strip's int16 levels are the int32 ones (|level| <= 408), every wide
    strip has the marker at its origin; a CTU-row band (row0, row1) widens alone;
    the oracle checks the mixed frame's luma."""
    torch = torch_dev
    from nano_hevc import gpu
    rng = np.random.default_rng(70 + qp)
    nf, w, h = 3, 208, 136                              # ragged CTUs; chroma pitch 104: 8-sample aligned
    sets = gpu.yuv420_plane_sets(nf, w, h)
    fe = gpu.yuv420_frame_elems(w, h)
    buf = np.clip(100 + rng.integers(-100, 101, size=nf * fe), 0, 255).astype(np.int16)
    buf[fe:2 * fe] = rng.integers(-32768, 32768, size=fe)   # frame 1: wide everywhere
    buf[2 * fe + 70 * w + 150] = 300                         # frame 2: one wide luma strip
    buf[2 * fe + w * h + 10 * (w // 2) + 5] = -3             # ... and one wide U strip
    d = torch.from_numpy(buf).cuda()
    for (ps, ctb, pid, luma) in ((sets[0], 32, 0, True), (sets[1], 16, 1, False)):
        lvl = torch.zeros(d.shape, dtype=torch.int32, device="cuda")
        rec = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
        _, _, tu = gpu.tu_pipeline_planes(d, ps, ctb, pid, 99, qp, luma, lvl=lvl, rec=rec)
        lc = torch.full(d.shape, 7, dtype=torch.int16, device="cuda")
        rc = torch.zeros(d.shape, dtype=torch.int16, device="cuda")
        _, _, tuc, spill = gpu.tu_pipeline_planes_compact(d, ps, ctb, pid, 99, qp, luma, lvl=lc, rec=rc)
        wide = gpu.tu_levels_widen(lc, spill, ps, ctb)
        assert torch.equal(tu, tuc) and torch.equal(rec, rc)
        lv, wv, cv = lvl.cpu().numpy(), wide.cpu().numpy(), lc.cpu().numpy()
        sw = 1024 // ctb
        for p_ in range(ps.planes_per_group * ps.num_groups):
            g, c = divmod(p_, ps.planes_per_group)
            off = ps.base + g * ps.group_stride + c * ps.plane_stride
            L = lv[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            W = wv[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            Cc = cv[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            S = buf[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            assert np.array_equal(W, L), (ctb, p_)
            for sy0 in range(0, ps.height, ctb):          # strips in groups of 4 share the narrow decision
                for sx0 in range(0, ps.width, sw):
                    blk = Cc[sy0:sy0 + ctb, sx0:sx0 + sw]
                    if blk[0, 0] == -32768:
                        continue
                    assert np.array_equal(blk, L[sy0:sy0 + ctb, sx0:sx0 + sw]) and np.abs(blk).max() <= 408
            if p_ == 0 and luma:                          # frame 0 is 8-bit: no marker anywhere
                assert not (Cc[::ctb, ::sw] == -32768).any()
            if p_ == 1 and luma:                          # frame 1: every strip marked
                assert (Cc[::ctb, ::sw] == -32768).all()
            if p_ == 2 and luma:
                el, er, et = O.tu_pipeline_plane(S.copy(), 32, 0, 99, qp, True)
                assert np.array_equal(W, el)
        # a band of CTU rows widens alone
        band = gpu.tu_levels_widen(lc, spill, ps, ctb, 1, 3)
        bv = band.cpu().numpy()
        for p_ in range(ps.planes_per_group * ps.num_groups):
            g, c = divmod(p_, ps.planes_per_group)
            off = ps.base + g * ps.group_stride + c * ps.plane_stride
            B = bv[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            L = lv[off:off + ps.height * ps.pitch].reshape(ps.height, ps.pitch)[:, :ps.width]
            assert np.array_equal(B[ctb:3 * ctb], L[ctb:3 * ctb]) and not B[:ctb].any() and not B[3 * ctb:].any()
