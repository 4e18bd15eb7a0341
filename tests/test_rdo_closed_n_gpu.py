"""GPU parity of the NxN 35-mode CLOSED-loop RDO:
``gpu.intra_rdo_closed_n`` at N = 4 (DST and DCT), 16 and 32 against the
pinned-oracle yardstick tests/rdo_closed_ref.py and the reference's recorded cases
(tests/golden/rdo_closed_n.npz).  Bar: modes, levels, recon and SSE bit-exact; every
output buffer is filled with a sentinel first.  8-bit sources say nothing at
N = 32 (§3.7a: the recon is a constant 128), so those cases use wide pictures.
No test provokes a stall."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdo_closed_ref as ref  # noqa: E402

SENTINEL = -12345
KINDS = [(4, True), (4, False), (16, False), (32, False)]


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


def _picture(h, w, seed, n):
    """8-bit at N = 4 / 16, wide at N = 32."""
    return ref.wide_picture(h, w, seed) if n == 32 else ref.picture(h, w, seed)


def _qp(n):
    return 4 if n == 32 else 22


def _plane_views(buf, sets):
    """Writable (h, w) views of every plane of ``sets`` inside the 1-D array ``buf``, set by set."""
    for s in sets:
        for g in range(s.num_groups):
            for c in range(s.planes_per_group):
                b = s.base + g * s.group_stride + c * s.plane_stride
                yield np.lib.stride_tricks.as_strided(buf[b:], (s.height, s.width),
                                                      (s.pitch * buf.itemsize, buf.itemsize))


def _expect(buf, sets, n, qp, dst):
    """The yardstick over plane sets: (modes, lvl, rec, sse per plane), SENTINEL wherever nothing is
    written -- levels outside full blocks, everything outside the plane rectangles."""
    lvl = np.full(buf.shape, SENTINEL, np.int32)
    rec = np.full(buf.shape, SENTINEL, np.int16)
    modes, sse = [], []
    for s, lv, rv in zip(_plane_views(buf, sets), _plane_views(lvl, sets), _plane_views(rec, sets)):
        m, _, _, t = ref.rdo_plane_closed(s, n, qp, dst, lvl=lv, rec=rv)
        modes.append(m.ravel())
        sse.append(t)
    return np.concatenate(modes) if modes else np.zeros(0, np.uint8), lvl, rec, np.array(sse, np.int64)


def _run(torch, gpu, buf, sets, n, qp, dst):
    """The kernels on the same buffer, outputs pre-filled with SENTINEL."""
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(buf.shape, SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full(buf.shape, SENTINEL, dtype=torch.int16, device="cuda")
    m, l, r, s = gpu.intra_rdo_closed_n(d, sets, n, qp, dst, lvl=lvl, rec=rec)
    assert l is lvl and r is rec
    torch.cuda.synchronize()
    return m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()


def _same(got, want):
    for name, g, w in zip(("modes", "lvl", "rec", "sse"), got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, f"{name}: {bad.size} of {g.size} differ, first at {bad[:4]}: " \
                              f"{g.ravel()[bad[:4]]} vs {w.ravel()[bad[:4]]}"


@functools.lru_cache(maxsize=None)
def _expect_cached(raw, shape, n, qp, dst):
    """One yardstick run per distinct (picture, N, QP, transform), shared between tests; read only."""
    from nano_hevc import gpu
    buf = np.frombuffer(raw, np.int16).copy()
    out = _expect(buf, [gpu.plane_set(0, shape[1], shape[0])], n, qp, dst)
    for a in out:
        a.setflags(write=False)
    return out


def _one_plane(torch, gpu, src, n, qp, dst):
    h, w = src.shape
    buf = np.ascontiguousarray(src).ravel()
    got = _run(torch, gpu, buf, [gpu.plane_set(0, w, h)], n, qp, dst)
    want = _expect_cached(buf.tobytes(), (h, w), n, qp, dst)
    _same(got, want)
    return want


# ------------------------------------------------------------------ 1. the reference's recorded cases

@pytest.mark.parametrize("k", range(4))
def test_recorded_reference_cases(torch, gpu, golden, k):
    g = golden("rdo_closed_n.npz")
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    src = g[f"c{k}_src"]
    h, w = src.shape
    got = _run(torch, gpu, np.ascontiguousarray(src).ravel(), [gpu.plane_set(0, w, h)], n, qp, dst)
    lvl = np.full((h, w), SENTINEL, np.int32)            # levels outside full blocks keep the caller's contents
    lvl[:h // n * n, :w // n * n] = g[f"c{k}_lvl"][:h // n * n, :w // n * n]
    want = (g[f"c{k}_modes"].ravel(), lvl.ravel(), g[f"c{k}_rec"].ravel(), np.array([g[f"c{k}_sse"]], np.int64))
    _same(got, want)


# ------------------------------------------------------------------ 2. three by three

@pytest.mark.parametrize("n,dst", KINDS)
def test_three_by_three_with_ragged_edges(torch, gpu, n, dst):
    """The smallest plane with a top-right wait, a carried top-left, a left column hand-off and a zero
    read past the last full block (the top-right of the last block column)."""
    src = _picture(3 * n + 2, 3 * n + 3, 1000 + n + dst, n)
    modes, lvl, rec, _ = _one_plane(torch, gpu, src, n, _qp(n), dst)
    assert modes.size == 9 and len(np.unique(modes)) >= 3 and np.count_nonzero(lvl[lvl != SENTINEL])
    assert len(np.unique(rec)) > 2


# ------------------------------------------------------------------ 3. narrow and short planes

@pytest.mark.parametrize("n,dst", KINDS)
def test_narrow_short_and_blockless_planes(torch, gpu, n, dst):
    qp = _qp(n)
    _one_plane(torch, gpu, _picture(3 * n + 1, n + 2, 1100 + n, n), n, qp, dst)      # one block wide: no top-right
    _one_plane(torch, gpu, _picture(n + 1, 3 * n + 2, 1110 + n, n), n, qp, dst)      # one block high: no wait at all
    for h, w in ((n - 1, 3 * n), (2 * n, n - 1)):                                    # no full block
        src = _picture(h, w, 1120 + n, n)
        m, l, r, s = _run(torch, gpu, src.ravel().copy(), [gpu.plane_set(0, w, h)], n, qp, dst)   # status 0: no raise
        assert m.size == 0 and (l == SENTINEL).all() and not r.any() and s.tolist() == [0]


# ------------------------------------------------------------------ 4. full-range int16

@pytest.mark.parametrize("n,dst,qp", [(4, True, 13), (16, False, 26), (32, False, 7)])
def test_full_range_int16(torch, gpu, n, dst, qp):
    """D8's int16 wrap in the interpolation, the wrapping residual / reconstruction adds, SSE past 2^32."""
    rng = np.random.default_rng(3000 + n + dst)
    src = rng.integers(-32768, 32768, (3 * n + 3, 3 * n + 5)).astype(np.int16)
    _, _, _, sse = _one_plane(torch, gpu, src, n, qp, dst)
    assert int(sse[0]) > 1 << 32


# ------------------------------------------------------------------ 5. ties go to the lowest mode

@pytest.mark.parametrize("n,dst", KINDS)
def test_flat_plane_every_block_ties_on_mode_0(torch, gpu, n, dst):
    """A flat plane at the border value 128: every prediction is 128, every residual 0, the recon stays
    128, so all 35 modes tie on every block.  (At another value the first block's coded residual makes
    the recon uneven and later blocks need not tie: that plane is compared with the yardstick alone.)"""
    src = np.full((2 * n + 1, 3 * n + 2), 128, np.int16)
    modes, lvl, _, sse = _one_plane(torch, gpu, src, n, 30, dst)
    assert not modes.any() and sse.tolist() == [0] and not lvl[lvl != SENTINEL].any()
    assert ref.tied_blocks(src, n, 30, dst).all()
    _one_plane(torch, gpu, np.full((2 * n + 1, 3 * n + 2), 77, np.int16), n, 30, dst)


# ------------------------------------------------------------------ 6. QP

@pytest.mark.parametrize("qp", [0, 17, 37, 51])
@pytest.mark.parametrize("n,dst", [(4, True), (16, False)])
def test_qp_range(torch, gpu, n, dst, qp):
    _one_plane(torch, gpu, ref.picture(2 * n, 3 * n, 500 + n), n, qp, dst)


def test_bad_arguments_raise_value_error(torch, gpu):
    d = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    s = [gpu.plane_set(0, 64, 64)]
    for n in (4, 8, 16, 32):
        for qp in (-1, 52):
            with pytest.raises(ValueError, match="qp"):
                gpu.intra_rdo_closed_n(d, s, n, qp)
    with pytest.raises(ValueError, match="block_size"):
        gpu.intra_rdo_closed_n(d, s, 12, 30)
    with pytest.raises(ValueError, match="use_dst"):
        gpu.intra_rdo_closed_n(d, s, 16, 30, use_dst=True)
    with pytest.raises(ValueError, match="nsets"):
        gpu.intra_rdo_closed_n(d, s * 9, 16, 30)


# ------------------------------------------------------------------ 7. layout and store forms

@pytest.mark.parametrize("n,dst", KINDS)
def test_layout_and_both_store_forms(torch, gpu, n, dst):
    """Pitch != width, two planes side by side per group x two groups with gaps, a base offset.  The
    same planes once with base, pitch and strides multiples of 8 (16-B row stores) and once with an
    odd base (element stores): each equals the yardstick, so they agree.  Every element outside the
    plane rectangles keeps the sentinel; recon inside a rectangle but outside full blocks is 0."""
    qp = _qp(n)
    w, h = 2 * n + 3, 2 * n + 2                      # 2 x 2 full blocks, ragged both ways
    pitch = (2 * w + 8 + 7) // 8 * 8                 # two planes side by side in a row, and a gap
    pstride = (w + 7) // 8 * 8                       # the second plane starts inside the first one's pitch
    gstride = h * pitch + 16
    pics = [_picture(h, w, 1200 + 10 * n + k, n) for k in range(4)]
    outs = []
    for base in (8, 5):
        s = gpu.plane_set(base, w, h, pitch, 2, 2, pstride, gstride)
        total = base + gstride + (h - 1) * pitch + pstride + w + 3
        rng = np.random.default_rng(600 + n)
        buf = rng.integers(0, 256, total).astype(np.int16)      # noise everywhere, gaps included
        for v, p in zip(_plane_views(buf, [s]), pics):
            v[:] = p
        got, want = _run(torch, gpu, buf, [s], n, qp, dst), _expect(buf, [s], n, qp, dst)
        _same(got, want)
        assert got[0].size == 16 and got[3].size == 4
        assert (want[2] == SENTINEL).sum() == total - 4 * w * h               # rec: the whole rectangles written
        assert (want[1] == SENTINEL).sum() == total - 4 * 4 * n * n           # lvl: full blocks only
        assert (want[2] == 0).sum() >= 4 * (w * h - 4 * n * n)
        outs.append(tuple(a[base:] if a.size == total else a for a in got))
    _same(outs[1], outs[0])


def test_eight_sets_of_0_to_3_block_rows(torch, gpu):
    n, qp = 16, 20
    # (h, w, planes per group, groups); set 2 is narrower than a block, set 5 has no group
    shapes = [(16, 33, 1, 1), (50, 17, 1, 2), (40, 15, 1, 1), (15, 40, 1, 1), (33, 32, 2, 1), (20, 20, 1, 0),
              (48, 16, 1, 1), (17, 49, 1, 1)]
    sets, off = [], 3
    for h, w, ppg, ng in shapes:
        sets.append(gpu.plane_set(off, w, h, w, ppg, ng, h * w + 2, ppg * (h * w + 2) + 1))
        off += max(1, ng) * (ppg * (h * w + 2) + 1) + 5
    rng = np.random.default_rng(77)
    buf = rng.integers(0, 256, off).astype(np.int16)
    for k, v in enumerate(_plane_views(buf, sets)):
        v[:] = ref.picture(*v.shape, 700 + k)
    got, want = _run(torch, gpu, buf, sets, n, qp, False), _expect(buf, sets, n, qp, False)
    _same(got, want)
    assert got[0].size == 2 + 2 * 3 + 0 + 0 + 2 * 4 + 0 + 3 + 3 and got[3].size == 9 and got[3][3] == 0


# ------------------------------------------------------------------ 8. tickets recycle

@pytest.mark.parametrize("n,dst,planes", [(4, True, 8192), (16, False, 2048), (32, False, 1024)])
def test_more_rows_than_resident_workers(torch, gpu, n, dst, planes):
    """3 x ``planes`` block rows, at least 3x the workgroups the device can hold (32 x 256 one-wave
    workgroups; 8 per CU at 4 waves; 4 per CU at 33 KB of LDS): every worker claims further tickets.
    The planes cycle through 4 pictures; each must equal its picture's expected outputs."""
    qp, side = _qp(n), 3 * n
    pics = [_picture(side, side, 1300 + 10 * n + k, n) for k in range(4)]
    want = [_expect_cached(p.tobytes(), (side, side), n, qp, dst) for p in pics]
    buf = np.concatenate([p.ravel() for p in pics] * (planes // 4))
    m, l, r, s = _run(torch, gpu, buf, [gpu.plane_set(0, side, side, side, 1, planes, 0, side * side)], n, qp, dst)
    for name, g, k in (("modes", m, 0), ("lvl", l, 1), ("rec", r, 2), ("sse", s, 3)):
        g = g.reshape(planes // 4, 4, -1)
        for p in range(4):
            bad = np.flatnonzero((g[:, p] != want[p][k].ravel()).any(axis=1))
            assert bad.size == 0, f"{name}: {bad.size} planes of picture {p} differ, first {4 * bad[:4] + p}"


# ------------------------------------------------------------------ 9. block_size 8 forwards

def test_block_size_8_is_the_existing_path(torch, gpu):
    rng = np.random.default_rng(8)
    sets = [gpu.plane_set(0, 40, 24, 40, 1, 2, 0, 24 * 40 + 24 * 20), gpu.plane_set(24 * 40, 20, 12, 20, 2, 2, 240,
                                                                                     24 * 40 + 24 * 20)]
    buf = rng.integers(0, 256, 2 * (24 * 40 + 24 * 20)).astype(np.int16)
    d = torch.from_numpy(buf).cuda()
    a = gpu.intra_rdo_closed_n(d, sets, 8, 27)
    b = gpu.intra_rdo_closed(d, sets, 27)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].numel() == 2 * 15 + 4 * 2 and int(a[3].sum()) > 0
