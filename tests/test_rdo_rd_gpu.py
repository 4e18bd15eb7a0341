"""GPU parity of the 35-mode RDO with a rate term:
``gpu.intra_rdo_rd_planes_n`` / ``gpu.intra_rdo_rd_closed_n`` at N = 4 (DST and DCT), 8,
16 and 32 against the pinned-oracle yardstick tests/rdo_rd_ref.py.  Bar: modes,
levels, recon and the three stats (sum J, sum D, sum R) bit-exact; every output
buffer is filled with a sentinel first.  The lambdas come from rdo_rd_ref.TABLE: at
them the mode map differs from lambda = 0's in at least 3 of 9 blocks, so a kernel
that ignores lambda fails.  No test provokes a stall or a fault."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdo_closed_ref  # noqa: E402
import rdo_rd_ref as ref  # noqa: E402
import rdo_ref  # noqa: E402

SENTINEL = -12345
KINDS = ref.KINDS
LOOPS = [False, True]     # closed


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


def _expect(buf, sets, n, qp, lam, dst, closed):
    """The yardstick over plane sets: (modes, lvl, rec, stats (planes, 3)), SENTINEL wherever nothing is
    written -- outside full blocks (closed loop: levels only), outside the plane rectangles."""
    lvl = np.full(buf.shape, SENTINEL, np.int32)
    rec = np.full(buf.shape, SENTINEL, np.int16)
    modes, stats = [], []
    walk = ref.rd_plane_closed if closed else ref.rd_plane
    for s, lv, rv in zip(_plane_views(buf, sets), _plane_views(lvl, sets), _plane_views(rec, sets)):
        m, _, _, st, _ = walk(s, n, qp, lam, dst, lvl=lv, rec=rv)
        modes.append(m.ravel())
        stats.append(st)
    return (np.concatenate(modes) if modes else np.zeros(0, np.uint8), lvl, rec,
            np.array(stats, np.int64).reshape(-1, 3))


def _run(torch, gpu, buf, sets, n, qp, lam, dst, closed):
    """The kernels on the same buffer, outputs pre-filled with SENTINEL."""
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(buf.shape, SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full(buf.shape, SENTINEL, dtype=torch.int16, device="cuda")
    fn = gpu.intra_rdo_rd_closed_n if closed else gpu.intra_rdo_rd_planes_n
    m, l, r, s = fn(d, sets, n, qp, lam, dst, lvl=lvl, rec=rec)
    assert l is lvl and r is rec and s.dtype == torch.int64 and s.dim() == 2 and s.shape[1] == 3
    torch.cuda.synchronize()
    return m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()


def _same(got, want):
    for name, g, w in zip(("modes", "lvl", "rec", "stats"), got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, f"{name}: {bad.size} of {g.size} differ, first at {bad[:4]}: " \
                              f"{g.ravel()[bad[:4]]} vs {w.ravel()[bad[:4]]}"


@functools.lru_cache(maxsize=None)
def _expect_cached(raw, shape, n, qp, lam, dst, closed):
    """One yardstick run per distinct (picture, N, QP, lambda, transform, loop), shared between tests; read only."""
    from nano_hevc import gpu
    buf = np.frombuffer(raw, np.int16).copy()
    out = _expect(buf, [gpu.plane_set(0, shape[1], shape[0])], n, qp, lam, dst, closed)
    for a in out:
        a.setflags(write=False)
    return out


def _one_plane(torch, gpu, src, n, qp, lam, dst, closed):
    h, w = src.shape
    buf = np.ascontiguousarray(src).ravel()
    got = _run(torch, gpu, buf, [gpu.plane_set(0, w, h)], n, qp, lam, dst, closed)
    want = _expect_cached(buf.tobytes(), (h, w), n, qp, lam, dst, closed)
    _same(got, want)
    return want


def _table(n, dst):
    wide, qp, lam = ref.TABLE[(n, dst)]
    return qp, lam


# ------------------------------------------------------------------ 1. three by three, ragged

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("n,dst", KINDS)
def test_three_by_three_ragged_at_three_lambdas(torch, gpu, n, dst, closed):
    """(3N+2) x (3N+3): the top-right wait, the carried top-left, the zero read past the last full block.
    The table's lambda moves >= 3 of the 9 decisions away from lambda = 0's (asserted from the
    yardstick), so these cases fail on a kernel that ignores lambda."""
    qp, lam = _table(n, dst)
    src = ref.table_picture(n, dst)
    want = {l: _one_plane(torch, gpu, src, n, qp, l, dst, closed) for l in (0, lam, ref.LAM_MAX)}
    assert want[0][0].size == 9 and int((want[0][0] != want[lam][0]).sum()) >= 3
    assert want[0][3][0, 0] == want[0][3][0, 1] and want[0][3][0, 2] >= 9       # lambda 0: J = D


# ------------------------------------------------------------------ 2. lambda = 0 is the existing decision

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n,dst", KINDS)
def test_lambda_0_equals_the_existing_entry_points(torch, gpu, n, dst, wide, closed):
    """Modes, levels and recon of intra_rdo_planes_n / intra_rdo_closed_n on the device, bit for bit, and
    sum J = sum D = their SSE.  At N = 8 this compares the N-lane chains with the packed 8x8 kernels."""
    pic = rdo_closed_ref.wide_picture if wide else rdo_ref.picture
    h, w = 3 * n + 1, 2 * n + 3
    buf = pic(h, w, 1400 + n + dst).ravel().copy()
    s = [gpu.plane_set(0, w, h)]
    qp = 4 if wide else 22
    got = _run(torch, gpu, buf, s, n, qp, 0, dst, closed)
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(buf.shape, SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full(buf.shape, SENTINEL, dtype=torch.int16, device="cuda")
    m, l, r, sse = (gpu.intra_rdo_closed_n if closed else gpu.intra_rdo_planes_n)(d, s, n, qp, dst, lvl=lvl, rec=rec)
    torch.cuda.synchronize()
    stats = np.array([[int(sse[0]), int(sse[0]), got[3][0, 2]]], np.int64)
    _same(got, (m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), stats))
    assert 6 <= got[3][0, 2] <= 6 * (n * n + 1)
    if wide:     # an 8-bit picture may code nothing at the large sizes (§3.7a)
        assert got[3][0, 2] > 6 and np.count_nonzero(got[1][got[1] != SENTINEL])


# ------------------------------------------------------------------ 3. decodable

@pytest.mark.parametrize("n,dst", KINDS)
def test_the_closed_rd_stream_decodes_to_its_recon(torch, gpu, n, dst):
    qp, lam = _table(n, dst)
    src = ref.table_picture(n, dst)
    h, w = src.shape
    s = [gpu.plane_set(0, w, h)]
    d = torch.from_numpy(src.ravel().copy()).cuda()
    modes, lvl, rec, _ = gpu.intra_rdo_rd_closed_n(d, s, n, qp, lam, dst)
    out = torch.full((h * w,), SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.intra_decode_closed_n(modes, lvl, s, n, qp, dst, rec=out)
    torch.cuda.synchronize()
    assert torch.equal(dec, rec) and len(np.unique(rec.cpu().numpy())) > 2


# ------------------------------------------------------------------ 4. full-range int16

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("n,dst,qp", [(4, True, 13), (4, False, 13), (8, False, 20), (16, False, 26), (32, False, 7)])
def test_full_range_int16_at_the_largest_lambda(torch, gpu, n, dst, qp, closed):
    """D8's int16 wrap, the wrapping residual / reconstruction adds, and D, lambda * R and J past 2^32."""
    rng = np.random.default_rng(3000 + n + dst)
    src = rng.integers(-32768, 32768, (3 * n + 3, 3 * n + 5)).astype(np.int16)
    stats = _one_plane(torch, gpu, src, n, qp, ref.LAM_MAX, dst, closed)[3]
    assert int(stats[0, 1]) > 1 << 32 and int(stats[0, 0]) > 1 << 32
    assert int(stats[0, 0]) == int(stats[0, 1]) + ref.LAM_MAX * int(stats[0, 2])


# ------------------------------------------------------------------ 5. ties go to the lowest mode

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("n,dst", KINDS)
def test_flat_planes_tie_on_mode_0(torch, gpu, n, dst, closed):
    """A flat plane at the border value 128: every mode has J = lambda on every block."""
    lam = 12345
    src = np.full((2 * n + 1, 3 * n + 2), 128, np.int16)
    modes, lvl, _, stats = _one_plane(torch, gpu, src, n, 30, lam, dst, closed)
    assert not modes.any() and stats.tolist() == [[6 * lam, 0, 6]] and not lvl[lvl != SENTINEL].any()
    assert (ref.rd_plane_closed if closed else ref.rd_plane)(src, n, 30, lam, dst)[4].all()
    _one_plane(torch, gpu, np.full((2 * n + 1, 3 * n + 2), 77, np.int16), n, 30, lam, dst, closed)


# ------------------------------------------------------------------ 6. layout and store forms

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("n,dst", KINDS)
def test_layout_and_both_store_forms(torch, gpu, n, dst, closed):
    """Pitch != width, two planes side by side per group x two groups with gaps, a base offset: once with
    base, pitch and strides multiples of 8 (16-B row stores), once with an odd base (element stores).
    Every element outside the plane rectangles keeps the sentinel."""
    qp, lam = _table(n, dst)
    w, h = 2 * n + 3, 2 * n + 2                      # 2 x 2 full blocks, ragged both ways
    pitch = (2 * w + 8 + 7) // 8 * 8                 # two planes side by side in a row, and a gap
    pstride = (w + 7) // 8 * 8                       # the second plane starts inside the first one's pitch
    gstride = h * pitch + 16
    pics = [ref.table_picture(n, dst, h, w) + k for k in range(4)]
    outs = []
    for base in (8, 5):
        s = gpu.plane_set(base, w, h, pitch, 2, 2, pstride, gstride)
        total = base + gstride + (h - 1) * pitch + pstride + w + 3
        rng = np.random.default_rng(600 + n)
        buf = rng.integers(0, 256, total).astype(np.int16)      # noise everywhere, gaps included
        for v, p in zip(_plane_views(buf, [s]), pics):
            v[:] = p
        got, want = _run(torch, gpu, buf, [s], n, qp, lam, dst, closed), _expect(buf, [s], n, qp, lam, dst, closed)
        _same(got, want)
        assert got[0].size == 16 and got[3].shape == (4, 3)
        assert (want[1] == SENTINEL).sum() == total - 4 * 4 * n * n           # lvl: full blocks only
        assert (want[2] == SENTINEL).sum() == total - 4 * (w * h if closed else 4 * n * n)
        outs.append(tuple(a[base:] if a.size == total else a for a in got))
    _same(outs[1], outs[0])


# ------------------------------------------------------------------ 7. narrow, short and block-less planes

@pytest.mark.parametrize("n,dst", KINDS)
def test_narrow_short_and_blockless_planes_closed(torch, gpu, n, dst):
    qp, lam = _table(n, dst)
    _one_plane(torch, gpu, ref.table_picture(n, dst, 3 * n + 1, n + 2), n, qp, lam, dst, True)   # one block wide
    _one_plane(torch, gpu, ref.table_picture(n, dst, n + 1, 3 * n + 2), n, qp, lam, dst, True)   # one block high
    for h, w in ((n - 1, 3 * n), (2 * n, n - 1)):                                                # no full block
        src = ref.table_picture(n, dst, h, w)
        for closed in LOOPS:
            m, l, r, s = _run(torch, gpu, src.ravel().copy(), [gpu.plane_set(0, w, h)], n, qp, lam, dst, closed)
            assert m.size == 0 and (l == SENTINEL).all() and s.tolist() == [[0, 0, 0]]
            assert not r.any() if closed else (r == SENTINEL).all()


@pytest.mark.parametrize("closed", LOOPS)
def test_eight_sets_of_0_to_3_block_rows(torch, gpu, closed):
    n, qp, lam = 8, 4, 10 ** 4
    # (h, w, planes per group, groups); set 2 is narrower than a block, set 5 has no group
    shapes = [(8, 17, 1, 1), (25, 9, 1, 2), (20, 7, 1, 1), (7, 20, 1, 1), (17, 16, 2, 1), (10, 10, 1, 0),
              (24, 8, 1, 1), (9, 25, 1, 1)]
    sets, off = [], 3
    for h, w, ppg, ng in shapes:
        sets.append(gpu.plane_set(off, w, h, w, ppg, ng, h * w + 2, ppg * (h * w + 2) + 1))
        off += max(1, ng) * (ppg * (h * w + 2) + 1) + 5
    rng = np.random.default_rng(77)
    buf = rng.integers(0, 256, off).astype(np.int16)
    for k, v in enumerate(_plane_views(buf, sets)):
        v[:] = rdo_ref.picture(*v.shape, 700 + k)
    got, want = _run(torch, gpu, buf, sets, n, qp, lam, False, closed), _expect(buf, sets, n, qp, lam, False, closed)
    _same(got, want)
    assert got[0].size == 2 + 2 * 3 + 0 + 0 + 2 * 4 + 0 + 3 + 3 and got[3].shape == (9, 3)
    assert got[3][3].tolist() == [0, 0, 0] and got[3][4].tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 8. tickets recycle at the new N = 8 workers

def test_more_rows_than_resident_workers_at_8(torch, gpu):
    """3 x 2048 block rows of 224-lane workgroups, several times what the device holds: every worker
    claims further tickets.  The planes cycle through 4 pictures; each must equal its picture's outputs."""
    n, dst, planes, side = 8, False, 2048, 24
    qp, lam = _table(n, dst)
    pics = [rdo_ref.picture(side, side, 1300 + 10 * n + k) for k in range(4)]
    want = [_expect_cached(p.tobytes(), (side, side), n, qp, lam, dst, True) for p in pics]
    buf = np.concatenate([p.ravel() for p in pics] * (planes // 4))
    m, l, r, s = _run(torch, gpu, buf, [gpu.plane_set(0, side, side, side, 1, planes, 0, side * side)], n, qp, lam, dst,
                      True)
    for name, g, k in (("modes", m, 0), ("lvl", l, 1), ("rec", r, 2), ("stats", s, 3)):
        g = g.reshape(planes // 4, 4, -1)
        for p in range(4):
            bad = np.flatnonzero((g[:, p] != want[p][k].ravel()).any(axis=1))
            assert bad.size == 0, f"{name}: {bad.size} planes of picture {p} differ, first {4 * bad[:4] + p}"


# ------------------------------------------------------------------ 9. QP

@pytest.mark.parametrize("closed", LOOPS)
@pytest.mark.parametrize("qp", [0, 17, 37, 51])
@pytest.mark.parametrize("n,dst", [(4, True), (8, False)])
def test_qp_range(torch, gpu, n, dst, qp, closed):
    _one_plane(torch, gpu, rdo_ref.picture(2 * n, 3 * n, 500 + n), n, qp, 700, dst, closed)


# ------------------------------------------------------------------ 10. bad arguments

def test_bad_arguments_raise_value_error(torch, gpu):
    d = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    s = [gpu.plane_set(0, 64, 64)]
    for fn in (gpu.intra_rdo_rd_planes_n, gpu.intra_rdo_rd_closed_n):
        for n in (4, 8, 16, 32):
            for qp in (-1, 52):
                with pytest.raises(ValueError, match="qp"):
                    fn(d, s, n, qp, 10)
            for lam in (-1, 2 ** 31, 2 ** 40):
                with pytest.raises(ValueError, match="lambda"):
                    fn(d, s, n, 30, lam)
        with pytest.raises(ValueError, match="block_size"):
            fn(d, s, 12, 30, 10)
        with pytest.raises(ValueError, match="use_dst"):
            fn(d, s, 16, 30, 10, use_dst=True)
        with pytest.raises(ValueError, match="nsets"):
            fn(d, s * 9, 16, 30, 10)
        with pytest.raises(ValueError, match="smaller"):
            fn(d, s, 16, 30, 10, lvl=torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="pitch"):
        gpu.intra_rdo_rd_plane_n(d.reshape(64, 64), 16, 30, 10, pitch=60)
    m, l, r, st = gpu.intra_rdo_rd_plane_n(d.reshape(64, 64), 16, 30, 10, pitch=72)
    torch.cuda.synchronize()
    assert m.shape == (4, 4) and l.shape == r.shape == (64, 64) and st.shape == (1, 3)
