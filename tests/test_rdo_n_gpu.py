"""GPU parity of the NxN 35-mode open-loop RDO:
``gpu.intra_rdo_planes_n`` / ``intra_rdo_plane_n`` at N = 4 (DST and DCT), 16 and 32
against the pinned-oracle yardstick tests/rdo_ref.py and the reference's recorded
cases (tests/golden/rdo_n.npz).  Bar: modes, levels, recon and SSE bit-exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdo_ref  # noqa: E402

SENTINEL = -12345
KINDS = [(4, True), (4, False), (16, False), (32, False)]
RAGGED = {4: (23, 38), 16: (53, 70), 32: (70, 101)}


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


def _plane_views(buf, sets):
    """Writable (h, w) views of every plane of ``sets`` inside the 1-D array ``buf``, set by set."""
    for s in sets:
        for g in range(s.num_groups):
            for c in range(s.planes_per_group):
                b = s.base + g * s.group_stride + c * s.plane_stride
                yield np.lib.stride_tricks.as_strided(buf[b:], (s.height, s.width),
                                                      (s.pitch * buf.itemsize, buf.itemsize))


def _expect(buf, sets, n, qp, dst):
    """The yardstick over plane sets: (modes, lvl, rec, sse per plane), SENTINEL wherever nothing is written."""
    lvl = np.full(buf.shape, SENTINEL, np.int32)
    rec = np.full(buf.shape, SENTINEL, np.int16)
    modes, sse = [], []
    for s, lv, rv in zip(_plane_views(buf, sets), _plane_views(lvl, sets), _plane_views(rec, sets)):
        m, _, _, t = rdo_ref.rdo_plane(s, n, qp, dst, lvl=lv, rec=rv)
        modes.append(m.ravel())
        sse.append(t)
    return np.concatenate(modes) if modes else np.zeros(0, np.uint8), lvl, rec, np.array(sse, np.int64)


def _run(torch, gpu, buf, sets, n, qp, dst):
    """The kernels on the same buffer, outputs pre-filled with SENTINEL."""
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(buf.shape, SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full(buf.shape, SENTINEL, dtype=torch.int16, device="cuda")
    m, l, r, s = gpu.intra_rdo_planes_n(d, sets, n, qp, dst, lvl=lvl, rec=rec)
    assert l is lvl and r is rec
    torch.cuda.synchronize()
    return m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()


def _same(got, want):
    for name, g, w in zip(("modes", "lvl", "rec", "sse"), got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, f"{name}: {bad.size} of {g.size} differ, first at {bad[:4]}: " \
                              f"{g.ravel()[bad[:4]]} vs {w.ravel()[bad[:4]]}"


def _one_plane(torch, gpu, src, n, qp, dst):
    h, w = src.shape
    buf = np.ascontiguousarray(src).ravel()
    sets = [gpu.plane_set(0, w, h)]
    got, want = _run(torch, gpu, buf, sets, n, qp, dst), _expect_cached(buf.tobytes(), (h, w), n, qp, dst)
    _same(got, want)
    return want


@functools.lru_cache(maxsize=None)
def _expect_cached(raw, shape, n, qp, dst):
    """One yardstick run per distinct (picture, N, QP, transform), shared between tests."""
    from nano_hevc import gpu
    buf = np.frombuffer(raw, np.int16).copy()
    return _expect(buf, [gpu.plane_set(0, shape[1], shape[0])], n, qp, dst)


# ------------------------------------------------------------------ 1. the reference's recorded cases

@pytest.mark.parametrize("k", range(4))
def test_recorded_reference_cases(torch, gpu, golden, k):
    g = golden("rdo_n.npz")
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    src = g[f"c{k}_src"]
    h, w = src.shape
    m, l, r, s = gpu.intra_rdo_plane_n(torch.from_numpy(src).cuda(), n, qp, dst)
    torch.cuda.synchronize()
    assert m.shape == (h // n, w // n)
    want = (g[f"c{k}_modes"], g[f"c{k}_lvl"], g[f"c{k}_rec"], np.array([g[f"c{k}_sse"]], np.int64))
    _same((m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()), want)
    # the same plane with rows pitch samples apart
    m, l, r, s = gpu.intra_rdo_plane_n(torch.from_numpy(src).cuda(), n, qp, dst, pitch=w + 3)
    torch.cuda.synchronize()
    _same((m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()), want)


# ------------------------------------------------------------------ 2. edges of a ragged picture

@pytest.mark.parametrize("n,dst,qp", [(4, True, 27), (4, False, 24), (16, False, 12), (32, False, 6)])
def test_ragged_picture_edges(torch, gpu, n, dst, qp):
    """Plane border (128), interior blocks, a 2N top reference truncated at the right edge, a left
    reference truncated at the bottom, skipped partial blocks."""
    h, w = RAGGED[n]
    assert h % n and w % n     # partial blocks; the last block column / row has truncated 2N references
    src = rdo_ref.picture(h, w, 2000 + n + dst)
    modes, lvl, _, _ = _one_plane(torch, gpu, src, n, qp, dst)
    assert len(np.unique(modes)) >= 3 and np.count_nonzero(lvl[lvl != SENTINEL])
    if n <= 16:
        assert ((modes >= 2) & (modes <= 17)).any() and (modes >= 18).any()


# ------------------------------------------------------------------ 3. full-range int16

@pytest.mark.parametrize("n,dst,qp", [(4, True, 13), (4, False, 40), (16, False, 26), (32, False, 7)])
def test_full_range_int16(torch, gpu, n, dst, qp):
    """D8's int16 wrap in the interpolation, the wrapping residual / reconstruction adds, SSE past 2^32."""
    rng = np.random.default_rng(3000 + n + dst)
    src = rng.integers(-32768, 32768, (37, 70)).astype(np.int16)
    _, _, _, sse = _one_plane(torch, gpu, src, n, qp, dst)
    if n == 32:
        assert int(sse[0]) > 1 << 32


# ------------------------------------------------------------------ 4. ties go to the lowest mode

@pytest.mark.parametrize("n,dst", KINDS)
def test_flat_plane_ties(torch, gpu, n, dst):
    src = np.full((40, 72), 77, np.int16)
    modes, _, _, _ = _one_plane(torch, gpu, src, n, 30, dst)
    assert set(np.unique(modes).tolist()) == ({0, 2} if n == 32 else {0, 2, 26})


# ------------------------------------------------------------------ 5. QP

@pytest.mark.parametrize("qp", [0, 4, 17, 37, 51])
@pytest.mark.parametrize("n,dst", [(4, True), (16, False)])
def test_qp_range(torch, gpu, n, dst, qp):
    src = rdo_ref.picture(2 * n, 3 * n, 500 + n)
    _one_plane(torch, gpu, src, n, qp, dst)


@pytest.mark.parametrize("qp", [-1, 52])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_qp_outside_0_51_is_refused(torch, gpu, n, qp):
    d = torch.zeros((64, 64), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError, match="qp"):
        gpu.intra_rdo_plane_n(d, n, qp)
    with pytest.raises(ValueError, match="block_size"):
        gpu.intra_rdo_plane_n(d, 12, 30)
    with pytest.raises(ValueError, match="use_dst"):
        gpu.intra_rdo_plane_n(d, 16, 30, use_dst=True)


# ------------------------------------------------------------------ 6. layout

@pytest.mark.parametrize("n,dst,qp", [(4, True, 22), (16, False, 17), (32, False, 5)])
def test_layout_pitch_base_groups_and_untouched_samples(torch, gpu, n, dst, qp):
    """Pitch != width, a base offset, two planes per group x two groups with gaps, the last plane ending at
    the buffer's last element; every element outside full blocks keeps the sentinel."""
    w, h = 2 * n + 3, n + 2                       # 2 x 1 full blocks, ragged both ways
    pitch = w + 5
    span = (h - 1) * pitch + w
    base, pstride = 7, span + 9
    gstride = 2 * pstride + 11
    total = base + gstride + pstride + span       # the last plane's last sample is the last element
    s = gpu.plane_set(base, w, h, pitch, 2, 2, pstride, gstride)
    rng = np.random.default_rng(600 + n)
    buf = rng.integers(0, 256, total).astype(np.int16)   # noise everywhere, gaps included
    for k, v in enumerate(_plane_views(buf, [s])):
        v[:] = rdo_ref.picture(h, w, 610 + k)
    got, want = _run(torch, gpu, buf, [s], n, qp, dst), _expect(buf, [s], n, qp, dst)
    _same(got, want)
    assert got[0].size == 8 and got[3].size == 4
    assert (want[1] == SENTINEL).sum() == total - 4 * 2 * n * n        # the comparison covers the untouched samples


def test_eight_sets_one_without_a_block(torch, gpu):
    n, qp = 16, 20
    sizes = [(16, 16), (33, 17), (15, 40), (16, 32), (32, 16), (20, 20), (16, 16), (17, 49)]   # (h, w); set 2 holds no block
    sets, off = [], 3
    for h, w in sizes:
        sets.append(gpu.plane_set(off, w, h))
        off += h * w + 5
    rng = np.random.default_rng(77)
    buf = rng.integers(0, 256, off).astype(np.int16)
    for k, v in enumerate(_plane_views(buf, sets)):
        v[:] = rdo_ref.picture(*v.shape, 700 + k)
    got, want = _run(torch, gpu, buf, sets, n, qp, False), _expect(buf, sets, n, qp, False)
    _same(got, want)
    assert got[0].size == 1 + 2 + 0 + 2 + 2 + 1 + 1 + 3 and got[3].size == 8 and got[3][2] == 0
    with pytest.raises(ValueError, match="nsets"):
        gpu.intra_rdo_planes_n(torch.from_numpy(buf).cuda(), sets + [sets[0]], n, qp)


# ------------------------------------------------------------------ 7. block counts past one workgroup's share

@pytest.mark.parametrize("n,dst,shape", [(4, True, (20, 36)), (4, False, (12, 60)), (16, False, (16, 83)),
                                         (32, False, (32, 96))])
def test_block_count_not_a_multiple_of_the_workgroup_share(torch, gpu, n, dst, shape):
    """45 blocks of 4x4 against 7 per workgroup, 5 of 16x16 against 2, 3 of 32x32 against 1."""
    h, w = shape
    assert ((h // n) * (w // n)) % {4: 7, 16: 2, 32: 2}[n] != 0
    _one_plane(torch, gpu, rdo_ref.picture(h, w, 800 + n + dst), n, 9 if n == 32 else 25, dst)


# ------------------------------------------------------------------ 8. store forms

@pytest.mark.parametrize("n,dst", KINDS)
def test_vector_and_element_store_forms_agree(torch, gpu, n, dst):
    """16-B row stores (base and pitch multiples of 8) against element stores (odd base): the same picture."""
    h, w = 2 * n, 3 * n + (8 - (3 * n) % 8) % 8 + 8
    src = rdo_ref.picture(h, w, 900 + n)
    qp = 8 if n == 32 else 21
    outs = []
    for base in (0, 16, 5):
        buf = np.zeros(base + h * w, np.int16)
        buf[base:] = src.ravel()
        m, l, r, s = _run(torch, gpu, buf, [gpu.plane_set(base, w, h)], n, qp, dst)
        assert (l[:base] == SENTINEL).all() and (r[:base] == SENTINEL).all()
        outs.append((m, l[base:], r[base:], s))
    _same(outs[1], outs[0])
    _same(outs[2], outs[0])
    _same(outs[0], _expect_cached(src.tobytes(), (h, w), n, qp, dst))


# ------------------------------------------------------------------ 9. block_size 8 forwards

def test_block_size_8_is_the_existing_path(torch, gpu):
    rng = np.random.default_rng(8)
    sets = [gpu.plane_set(0, 40, 24, 40, 1, 2, 0, 24 * 40 + 24 * 20), gpu.plane_set(24 * 40, 20, 12, 20, 2, 2, 240,
                                                                                     24 * 40 + 24 * 20)]
    buf = rng.integers(0, 256, 2 * (24 * 40 + 24 * 20)).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    a = gpu.intra_rdo_planes_n(d, sets, 8, 27)
    b = gpu.intra_rdo_planes(d, sets, 27)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].numel() == 2 * 15 + 4 * 2 and int(a[3].sum()) > 0
