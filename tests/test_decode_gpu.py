"""GPU parity of the closed-loop intra decoder: stage R
(``gpu.dequant_inv8x8``) and ``gpu.intra_decode_closed`` against the pinned oracle
(tests/decode_ref.py) and the reference's recorded outputs.  Bar: bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from decode_ref import decode, residual_block, residual_plane  # noqa: E402

SENTINEL = -12345


@pytest.fixture(scope="module")
def torch():
    import torch
    from nano_hevc import _lib
    assert _lib.device_count() > 0 and torch.cuda.is_available(), "no HIP device: the gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def gpu():
    from nano_hevc import gpu
    return gpu


def _full_range(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dtype)


def _plane_views(buf, sets):
    """Writable (h, w) views of every plane of ``sets`` inside the 1-D array ``buf``, set by set."""
    for s in sets:
        for g in range(s.num_groups):
            for c in range(s.planes_per_group):
                b = s.base + g * s.group_stride + c * s.plane_stride
                yield np.lib.stride_tricks.as_strided(buf[b:], (s.height, s.width),
                                                      (s.pitch * buf.itemsize, buf.itemsize))


def _stage_r(torch, gpu, lvl, sets, qp):
    out = torch.full(lvl.shape, SENTINEL, dtype=torch.int16, device="cuda")
    r = gpu.dequant_inv8x8(torch.from_numpy(lvl).cuda(), sets, qp, out=out)
    assert r is out
    return out.cpu().numpy()


# ------------------------------------------------------------------ 1. stage R, full range

@pytest.mark.parametrize("qp", [0, 5, 23, 24, 51, -3, 60])
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_stage_r_full_range(torch, gpu, dtype, qp):
    rng = np.random.default_rng(1000 + qp + (7 if dtype is np.int32 else 0))
    lvl = _full_range(rng, (8, 512), dtype)
    want = np.concatenate([residual_block(lvl[:, x:x + 8], qp) for x in range(0, 512, 8)], axis=1)
    assert len(np.unique(want)) > 1000   # no clip in the way: the outputs span int16
    got = _stage_r(torch, gpu, lvl, [gpu.plane_set(0, 512, 8)], qp)
    assert got.dtype == np.int16 and np.array_equal(got, want)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_stage_r_zero_and_single_values(torch, gpu, dtype):
    vals = [1, -1, 32767, -32767, -32768]
    if dtype is np.int32:
        vals += [2 ** 31 - 1, -(2 ** 31 - 1)]
    lvl = np.zeros((8, 8 * (2 * len(vals) + 1)), dtype)        # block 0 stays all zero
    for k, v in enumerate(vals):
        lvl[0, 8 * (1 + 2 * k)] = v                               # position (0, 0)
        lvl[7, 8 * (2 + 2 * k) + 7] = v                           # position (7, 7)
    for qp in (0, 23, 24, 41, 51):
        want = np.concatenate([residual_block(lvl[:, x:x + 8], qp) for x in range(0, lvl.shape[1], 8)], axis=1)
        got = _stage_r(torch, gpu, lvl, [gpu.plane_set(0, lvl.shape[1], 8)], qp)
        assert np.array_equal(got, want), qp
        assert not got[:, :8].any()
    zero = np.zeros((16, 24), dtype)
    assert not _stage_r(torch, gpu, zero, [gpu.plane_set(0, 24, 16)], 30).any()


# ------------------------------------------------------------------ 2. stage R, layouts

def _layout_cases(gpu):
    return {
        "aligned": (16 + 24 * 48, [gpu.plane_set(16, 40, 24, 48)]),                   # base, pitch multiples of 8
        "ragged": (3 + 29 * 37, [gpu.plane_set(3, 37, 29, 37)]),                      # 29 x 37, pitch 37, base 3
        "yuv_aligned": (2 * gpu.yuv420_frame_elems(32, 16), gpu.yuv420_plane_sets(2, 32, 16)),
        "yuv_scalar": (2 * gpu.yuv420_frame_elems(36, 24), gpu.yuv420_plane_sets(2, 36, 24)),
    }


@pytest.mark.parametrize("case", ["aligned", "ragged", "yuv_aligned", "yuv_scalar"])
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_stage_r_layouts(torch, gpu, dtype, case):
    n, sets = _layout_cases(gpu)[case]
    if case.startswith("yuv"):
        assert len(sets) == 2 and sets[1].planes_per_group == 2 and sets[1].num_groups == 2
    rng = np.random.default_rng(77)
    lvl = _full_range(rng, n, dtype)
    for qp in (22, 45):
        want = np.full(n, SENTINEL, np.int16)
        for src, dst in zip(_plane_views(lvl, sets), _plane_views(want, sets)):
            residual_plane(src, qp, dst)
        got = _stage_r(torch, gpu, lvl, sets, qp)
        assert np.array_equal(got, want), (case, qp)
        if case != "yuv_aligned":   # samples outside full blocks (and pitch gaps) keep the sentinel
            assert (want == SENTINEL).any()


def test_stage_r_forms_agree(torch, gpu):
    """The 16-byte-row form and the scalar form on the same blocks (the host picks by alignment)."""
    rng = np.random.default_rng(5)
    blocks = _full_range(rng, (24, 40), np.int16)
    res = []
    for base, pitch in ((16, 48), (3, 41)):
        buf = np.zeros(base + 24 * pitch, np.int16)
        next(_plane_views(buf, [gpu.plane_set(base, 40, 24, pitch)]))[:] = blocks
        out = _stage_r(torch, gpu, buf, [gpu.plane_set(base, 40, 24, pitch)], 33)
        res.append(next(_plane_views(out, [gpu.plane_set(base, 40, 24, pitch)])).copy())
    assert np.array_equal(res[0], res[1])


# ------------------------------------------------------------------ 3. recorded outputs

def _decode_gpu(torch, gpu, modes, lvl, qp, **kw):
    h, w = lvl.shape
    rec = gpu.intra_decode_closed(torch.from_numpy(np.ascontiguousarray(modes, np.uint8).ravel()).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(lvl, np.int32)).cuda(),
                                  [gpu.plane_set(0, w, h, w)], qp, **kw)
    return rec.cpu().numpy().reshape(h, w)


@pytest.mark.parametrize("tag", ["c3a", "c3b", "c3c"])
def test_decode_reference_recorded(torch, gpu, golden, tag):
    g = golden("closed.npz")
    got = _decode_gpu(torch, gpu, g[tag + "_modes"], g[tag + "_lvl"], int(g[tag + "_qp"]))
    assert np.array_equal(got, g[tag + "_rec"])


# ------------------------------------------------------------------ 4. every mode at every position class

@pytest.mark.parametrize("qp,amp,dens", [(0, 40, 1.0), (23, 3, 1.0), (37, 1, 0.3), (51, 1, 0.05)])
def test_decode_every_mode_every_position(torch, gpu, qp, amp, dens):
    h, w, nb = 293, 292, 36
    rng = np.random.default_rng(3)
    modes = rng.integers(0, 35, (nb, nb)).astype(np.uint8)
    modes[0, :] = np.arange(nb) % 35
    modes[:, 0] = np.arange(nb) % 35
    modes[:, -1] = (np.arange(nb) + 17) % 35
    lvl = (rng.integers(-amp, amp + 1, (h, w)) * (rng.random((h, w)) < dens)).astype(np.int32)
    want = decode(modes, lvl, qp)
    inside = want[:nb * 8, :nb * 8]
    railed = float(((inside == 0) | (inside == 255)).mean())
    print(f"QP {qp}: {100 * railed:.1f} % of the expected samples are 0 or 255, "
          f"{len(np.unique(inside))} distinct values")
    assert railed < 0.35   # the clip cannot hide a wrong prediction or residual
    got = _decode_gpu(torch, gpu, modes, lvl, qp)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 5. round trip on the device

@pytest.mark.parametrize("pad", [0, 13])
@pytest.mark.parametrize("qp", [22, 37])
def test_decode_round_trip_yuv420(torch, gpu, qp, pad):
    W, H, F = 64, 48, 2
    fs = gpu.yuv420_frame_elems(W, H) + pad
    sets = gpu.yuv420_plane_sets(F, W, H, frame_stride=fs if pad else None)
    assert len(sets) == 2 and (sets[1].width, sets[1].height) == (32, 24)
    rng = np.random.default_rng(40 + qp)
    src = rng.integers(0, 256, F * fs).astype(np.int16)
    modes, lvl, rec, _ = gpu.intra_rdo_closed(torch.from_numpy(src).cuda(), sets, qp)
    dec = gpu.intra_decode_closed(modes, lvl, sets, qp)
    assert torch.equal(dec, rec)
    dec = dec.cpu().numpy()
    for f in range(F):   # the Y planes against the oracle's closed loop and its decode
        y = src[f * fs:f * fs + W * H].reshape(H, W)
        mo, lo, ro, _ = O.intra_rdo_plane(y, qp, closed=True)
        want = decode(mo, lo, qp)
        assert np.array_equal(want, ro)
        assert np.array_equal(dec[f * fs:f * fs + W * H].reshape(H, W), want)


# ------------------------------------------------------------------ 6. narrowest shapes

@pytest.mark.parametrize("h,w", [(8, 8), (8, 40), (40, 8), (7, 7)])
def test_decode_narrowest_shapes(torch, gpu, h, w):
    rng = np.random.default_rng(h * 100 + w)
    modes = rng.integers(0, 35, (h // 8, w // 8)).astype(np.uint8)
    lvl = rng.integers(-3, 4, (h, w)).astype(np.int32)
    rec = torch.full((h, w), SENTINEL, dtype=torch.int16, device="cuda")
    got = _decode_gpu(torch, gpu, modes, lvl, 27, rec=rec)   # status 0: no exception
    assert np.array_equal(got, decode(modes, lvl, 27))
    if h < 8:
        assert not got.any()


# ------------------------------------------------------------------ 7. bad mode

def test_decode_bad_mode_is_value_error(torch, gpu):
    h = w = 128
    rng = np.random.default_rng(9)
    modes = rng.integers(0, 35, (16, 16)).astype(np.uint8)
    lvl = rng.integers(-2, 3, (h, w)).astype(np.int32)
    bad = modes.copy()
    bad[11, 5] = 35
    with pytest.raises(ValueError):
        _decode_gpu(torch, gpu, bad, lvl, 30)
    assert np.array_equal(_decode_gpu(torch, gpu, modes, lvl, 30), decode(modes, lvl, 30))


# ------------------------------------------------------------------ 8. caller buffers

def test_decode_caller_buffer_and_stream(torch, gpu):
    h, w = 45, 75
    rng = np.random.default_rng(12)
    modes = rng.integers(0, 35, (h // 8, w // 8)).astype(np.uint8)
    lvl = rng.integers(-4, 5, (h, w)).astype(np.int32)
    fresh = _decode_gpu(torch, gpu, modes, lvl, 25)
    assert np.array_equal(fresh, decode(modes, lvl, 25))
    rec = torch.full((h, w), SENTINEL, dtype=torch.int16, device="cuda")
    assert np.array_equal(_decode_gpu(torch, gpu, modes, lvl, 25, rec=rec), fresh)   # nothing relies on a zeroed rec
    rec2 = torch.full((h, w), SENTINEL, dtype=torch.int16, device="cuda")
    d_modes, d_lvl = torch.from_numpy(modes.ravel()).cuda(), torch.from_numpy(lvl).cuda()
    torch.cuda.synchronize()   # the inputs are ready before the side stream reads them
    side = torch.cuda.Stream()
    got = gpu.intra_decode_closed(d_modes, d_lvl, [gpu.plane_set(0, w, h, w)], 25, rec=rec2, stream=side)
    side.synchronize()
    assert got is rec2 and np.array_equal(got.cpu().numpy(), fresh)
