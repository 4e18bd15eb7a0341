"""GPU parity of config 4's TU-size search and map-driven encode (DESIGN.md §3.4a,
§4.4d): ``gpu.tu_rd_planes``, ``gpu.tu_rd_plane``, ``gpu.tu_rd_yuv420`` and
``gpu.tu_encode_map_planes`` against the yardstick composed from the pinned oracle
(tests/tu_rd_ref.py), the reference-composed records and the seeded GPU encoder.
Bar: bit-exact everywhere; every output is pre-filled with a sentinel and every byte
outside the plane rectangles must come back unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tu_decode_ref as R  # noqa: E402
import tu_rd_ref as T  # noqa: E402

S16, S32, S8 = -12345, -1234567, 0xA5
SEED = 2024
TAIL = 7   # sentinel bytes behind the last plane's map


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


_CHAINS = {}


def chains(src, qp, luma):
    """One per-TU cache per (picture, qp, luma): shared by every test that needs it."""
    key = (src.shape, src.tobytes(), qp, luma)
    if key not in _CHAINS:
        _CHAINS[key] = T.Chains(src, qp, luma)
    return _CHAINS[key]


def _planes(ps):
    for g in range(ps.num_groups):
        for c in range(ps.planes_per_group):
            yield g * ps.planes_per_group + c, ps.base + g * ps.group_stride + c * ps.plane_stride


def _view(buf, ps, off):
    return np.lib.stride_tricks.as_strided(buf[off:], (ps.height, ps.width), (ps.pitch * buf.itemsize, buf.itemsize))


def _outside(n, ps):
    m = np.ones(n, bool)
    for _, off in _planes(ps):
        _view(m, ps, off)[:] = False
    return m


class Layout:
    """Planes (a list of equal-shape 2-D int16 arrays) laid out as one plane set."""

    def __init__(self, gpu, planes, base=0, pad=0, ppg=1, gap=0):
        self.planes = planes
        h, w = planes[0].shape
        assert len(planes) % ppg == 0
        pitch = w + pad
        ps_ = h * pitch + gap
        self.ps = gpu.plane_set(base, w, h, pitch, ppg, len(planes) // ppg, ps_, ppg * ps_ + gap)
        self.n = base + len(planes) * ps_ + (len(planes) // ppg) * gap + 5
        self.src = np.full(self.n, 77, np.int16)
        for (pl, off), p in zip(_planes(self.ps), planes):
            _view(self.src, self.ps, off)[:] = p
        self.units = len(planes) * (h // 4) * (w // 4)
        self.outside = _outside(self.n, self.ps)

    def outputs(self, torch):
        return (torch.full((self.n,), S32, dtype=torch.int32, device="cuda"),
                torch.full((self.n,), S16, dtype=torch.int16, device="cuda"),
                torch.full((self.units + TAIL,), S8, dtype=torch.uint8, device="cuda"),
                torch.full((self.units + TAIL,), S8, dtype=torch.uint8, device="cuda"))

    def split(self, lvl, rec, tu, pm, stats):
        """Per-plane numpy results after the sentinel checks."""
        lvl, rec, tu, pm, stats = (t.cpu().numpy() for t in (lvl, rec, tu, pm, stats))
        assert (lvl[self.outside] == S32).all() and (rec[self.outside] == S16).all()
        assert (tu[self.units:] == S8).all() and (pm[self.units:] == S8).all()
        h4, w4 = self.ps.height // 4, self.ps.width // 4
        tu, pm = tu[:self.units].reshape(-1, h4, w4), pm[:self.units].reshape(-1, h4, w4)
        assert stats.shape == (len(self.planes), 3) and stats.dtype == np.int64
        return [(tu[pl], pm[pl], _view(lvl, self.ps, off).copy(), _view(rec, self.ps, off).copy(), stats[pl])
                for pl, off in _planes(self.ps)]


def check_search(torch, gpu, planes, ctb, qp, lam, luma, **layout):
    lay = Layout(gpu, planes, **layout)
    d_src = torch.from_numpy(lay.src).cuda()
    lvl, rec, tu, pm = lay.outputs(torch)
    out = gpu.tu_rd_planes(d_src, lay.ps, ctb, qp, lam, luma, lvl=lvl, rec=rec, tu=tu, pm=pm)
    assert out[0] is lvl and out[1] is rec and out[2] is tu and out[3] is pm
    got = lay.split(*out)
    for k, (p, g) in enumerate(zip(planes, got)):
        want = T.rd_plane(p, ctb, qp, lam, luma, chains=chains(p, qp, luma))
        for name, a, b in zip(("tu", "pm", "lvl", "rec", "stats"), g, want):
            assert np.array_equal(a, b), (name, k)
    return lay, d_src, got


def check_map(torch, gpu, planes, maps, ctb, qp, lam, luma, **layout):
    lay = Layout(gpu, planes, **layout)
    d_src = torch.from_numpy(lay.src).cuda()
    lvl, rec, _, pm = lay.outputs(torch)
    tu = np.full(lay.units + TAIL, S8, np.uint8)
    tu[:lay.units] = np.concatenate([m.ravel() for m in maps])
    d_tu = torch.from_numpy(tu).cuda()
    out = gpu.tu_encode_map_planes(d_src, d_tu, lay.ps, ctb, qp, lam, luma, lvl=lvl, rec=rec, pm=pm)
    assert out[0] is lvl and out[1] is rec and out[2] is pm
    assert np.array_equal(d_tu.cpu().numpy(), tu)   # the map is an input
    got = lay.split(out[0], out[1], d_tu, out[2], out[3])
    for k, (p, m, g) in enumerate(zip(planes, maps, got)):
        want = T.encode_map(p, m, ctb, qp, lam, luma, chains=chains(p, qp, luma))
        for name, a, b in zip(("pm", "lvl", "rec", "stats"), g[1:], want):
            assert np.array_equal(a, b), (name, k)
    return got


def rnd16(h, w, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (h, w)).astype(np.int16)


def noisy8(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = 128 + 60 * np.sin(x / 5 + y / 9) + 40 * np.cos(y / 3 - x / 11) + rng.integers(-6, 7, (h, w))
    return a.clip(0, 255).astype(np.int16)


# ------------------------------------------------------------------ the search

@pytest.mark.parametrize("k", range(4))
def test_recorded_search(torch, gpu, golden, k):
    g = golden("tu_rd.npz")
    ctb, luma, qp, lam = (int(g[f"c{k}_{n}"]) for n in ("ctb", "luma", "qp", "lam"))
    _, _, got = check_search(torch, gpu, [g[f"c{k}_src"]], ctb, qp, lam, bool(luma))
    for name, a in zip(("tu", "pm", "lvl", "rec", "stats"), got[0]):
        assert np.array_equal(a, g[f"c{k}_{name}"]), name


@pytest.mark.parametrize("qp,lam", T.QP_LAMBDA)
@pytest.mark.parametrize("luma", [True, False])
def test_mixed_fixture(torch, gpu, luma, qp, lam):
    h, w, ctb = (132, 164, 32) if luma else (68, 84, 16)
    _, _, got = check_search(torch, gpu, [T.mixed_picture(h, w)], ctb, qp, lam, luma)
    assert min(T.area_shares(got[0][0], ctb)) >= 0.05


@pytest.mark.parametrize("luma,ctb", [(True, 16), (False, 32)])
def test_mixed_fixture_crossed(torch, gpu, luma, ctb):
    check_search(torch, gpu, [T.mixed_picture(68, 84)], ctb, 22, 400, luma)


@pytest.mark.parametrize("ctb", [16, 32])
@pytest.mark.parametrize("h,w", [(36, 44), (68, 100), (20, 20), (4, 4), (4, 36), (36, 4)])
def test_shapes(torch, gpu, h, w, ctb):
    _, _, got = check_search(torch, gpu, [T.mixed_picture(h, w)], ctb, 22, 400, ctb == 32)
    assert R.valid(got[0][0], ctb)


@pytest.mark.parametrize("lam", [0, 2 ** 31 - 1])
@pytest.mark.parametrize("ctb", [16, 32])
def test_full_range_source(torch, gpu, ctb, lam):
    check_search(torch, gpu, [rnd16(64, 64, 900 + ctb)], ctb, 30, lam, True)


@pytest.mark.parametrize("ctb", [16, 32])
def test_ties(torch, gpu, ctb):
    _, _, got = check_search(torch, gpu, [np.full((64, 64), 128, np.int16)], ctb, 30, 0, True)
    assert (got[0][0] == int(np.log2(ctb))).all() and got[0][4].tolist()[:2] == [0, 0]
    _, _, got = check_search(torch, gpu, [np.full((96, 96), 90, np.int16)], ctb, 30, 0, True)
    tu, top = got[0][0], int(np.log2(ctb))
    assert (tu[-ctb // 4:, -ctb // 4:] == top).all() and (tu[0] != top).all() and (tu[:, 0] != top).all()   # border CTBs split


@pytest.mark.parametrize("ctb", [16, 32])
def test_layouts(torch, gpu, ctb):
    planes = [noisy8(36, 44, 50 + k) if k % 2 else T.mixed_picture(36, 44) for k in range(6)]
    planes[3] = rnd16(36, 44, 53)
    # padded pitch, non-zero base, two planes per group in three groups; rows not 8-B aligned, then aligned
    check_search(torch, gpu, planes, ctb, 27, 300, ctb == 32, base=3, pad=5, ppg=2, gap=9)
    check_search(torch, gpu, planes, ctb, 27, 300, ctb == 32, base=8, pad=4, ppg=2, gap=12)


def test_more_workgroups_than_are_resident(torch, gpu):
    kinds = [T.mixed_picture(132, 164)[y:y + 32, x:x + 32].copy() for y, x in ((0, 0), (0, 100), (80, 20), (96, 128))]
    kinds += [noisy8(32, 32, 3), rnd16(32, 32, 4), np.full((32, 32), 128, np.int16), noisy8(32, 32, 5)]
    planes = [kinds[k % 8] for k in range(1536)]   # one CTB, one workgroup each
    check_search(torch, gpu, planes, 32, 24, 500, True, ppg=2)


# ------------------------------------------------------------------ the map-driven encode

@pytest.mark.parametrize("ctb,luma,pid", [(32, True, 0), (16, False, 1), (16, True, 0), (32, False, 1)])
def test_encode_map_on_the_seeded_map(torch, gpu, ctb, luma, pid):
    h, w = 68, 100
    planes = [noisy8(h, w, 70 + pid), T.mixed_picture(h, w)]
    lay = Layout(gpu, planes, ppg=2)
    d_src = torch.from_numpy(lay.src).cuda()
    lvl, rec, tu = gpu.tu_pipeline_planes(d_src, lay.ps, ctb, pid, SEED, 27, luma)
    maps = list(tu.cpu().numpy())
    assert all(R.valid(m, ctb) for m in maps)
    got = check_map(torch, gpu, planes, maps, ctb, 27, 150, luma, ppg=2)
    lvl, rec = lvl.cpu().numpy(), rec.cpu().numpy()
    for (pl, off), g in zip(_planes(lay.ps), got):
        assert np.array_equal(g[2], _view(lvl, lay.ps, off)) and np.array_equal(g[3], _view(rec, lay.ps, off))
    _, _, best = check_search(torch, gpu, planes, ctb, 27, 150, luma, ppg=2)
    assert all(b[4][0] <= o[4][0] for b, o in zip(best, got))   # the search can only do better


@pytest.mark.parametrize("ctb", [16, 32])
def test_encode_map_on_the_chosen_map(torch, gpu, ctb):
    planes = [T.mixed_picture(68, 100), rnd16(68, 100, 17)]
    _, _, best = check_search(torch, gpu, planes, ctb, 22, 400, ctb == 32, ppg=2, pad=4)
    got = check_map(torch, gpu, planes, [b[0] for b in best], ctb, 22, 400, ctb == 32, ppg=2, pad=4)
    for b, g in zip(best, got):
        for name, x, y in zip(("pm", "lvl", "rec", "stats"), b[1:], g[1:]):
            assert np.array_equal(x, y), name


def _checkerboard(h, w, ctb):
    """Sizes per 16x16 quadrant in a pattern no seed produces; CTB 32: one whole CTB too."""
    m = np.zeros((h // 4, w // 4), np.uint8)
    for qy in range(h // 16):
        for qx in range(w // 16):
            m[4 * qy:4 * qy + 4, 4 * qx:4 * qx + 4] = (4, 3, 2)[(qx + 2 * qy) % 3]
    if ctb == 32:
        m[8:16, 0:8] = 5
    return m


@pytest.mark.parametrize("ctb", [16, 32])
def test_encode_map_on_hand_made_maps(torch, gpu, ctb):
    h, w = 64, 96
    planes = [T.mixed_picture(h, w)]
    top = int(np.log2(ctb))
    lay, d_src, best = check_search(torch, gpu, planes, ctb, 22, 400, True)
    best = best[0]
    seeded = gpu.tu_pipeline_planes(d_src, lay.ps, ctb, 0, SEED, 22, True)[2].cpu().numpy()[0]
    for m in (np.full((h // 4, w // 4), 2, np.uint8), np.full((h // 4, w // 4), top, np.uint8), seeded,
              _checkerboard(h, w, ctb)):
        assert R.valid(m, ctb)
        got = check_map(torch, gpu, planes, [m], ctb, 22, 400, True)[0]
        assert best[4][0] <= got[4][0]


@pytest.mark.parametrize("ctb", [16, 32])
def test_invalid_maps_raise_and_the_process_goes_on(torch, gpu, ctb):
    h, w = 72, 40   # 72 = 2 * 32 + 8 = 4 * 16 + 8: the last CTB row overhangs
    src = T.mixed_picture(h, w)
    ps = gpu.plane_set(0, w, h, w)
    d_src = torch.from_numpy(src.ravel().copy()).cuda()
    top = int(np.log2(ctb))
    good = np.full((h // 4, w // 4), 2, np.uint8)
    good[0:ctb // 4, 0:ctb // 4] = top
    bad = {}
    for name, v in (("one", 1), ("six", 6), ("above ctb", top + 1)):
        bad[name] = good.copy()
        bad[name][5, 5] = v
    bad["incomplete square"] = good.copy()
    bad["incomplete square"][1, 1] = 2
    bad["overhang"] = good.copy()
    bad["overhang"][16:18, 0:4] = 4   # a 16x16 square from unit row 16 leaves the plane's 18 unit rows
    want = T.encode_map(src, good, ctb, 30, 10, True)
    for name, m in bad.items():
        assert not R.valid(m, ctb), name
        with pytest.raises(ValueError):
            gpu.tu_encode_map_planes(d_src, torch.from_numpy(m).cuda(), ps, ctb, 30, 10, True)
        lvl, rec, pm, stats = gpu.tu_encode_map_planes(d_src, torch.from_numpy(good).cuda(), ps, ctb, 30, 10, True)
        assert np.array_equal(lvl.cpu().numpy().reshape(h, w), want[1]), name
        assert np.array_equal(rec.cpu().numpy().reshape(h, w), want[2]) and np.array_equal(pm.cpu().numpy()[0], want[0])
        assert np.array_equal(stats.cpu().numpy()[0], want[3])


# ------------------------------------------------------------------ yuv420, single plane, plumbing

def test_yuv420_equals_the_per_set_calls(torch, gpu):
    W, H, F = 64, 48, 2
    fe = gpu.yuv420_frame_elems(W, H)
    luma, chroma = gpu.yuv420_plane_sets(F, W, H)
    buf = np.concatenate([np.concatenate([noisy8(H, W, 30 + f).ravel(), T.mixed_picture(H // 2, W // 2).ravel(),
                                          noisy8(H // 2, W // 2, 40 + f).ravel()]) for f in range(F)])
    assert buf.size == F * fe
    d = torch.from_numpy(buf).cuda()
    lvl, rec, (tu_y, pm_y, st_y), (tu_c, pm_c, st_c) = gpu.tu_rd_yuv420(d, luma, chroma, 27, 200)
    l2, r2, tu, pm, st = gpu.tu_rd_planes(d, luma, 32, 27, 200, True)
    assert torch.equal(tu, tu_y) and torch.equal(pm, pm_y) and torch.equal(st, st_y)
    l2, r2, tu, pm, st = gpu.tu_rd_planes(d, chroma, 16, 27, 200, False, lvl=l2, rec=r2)
    assert torch.equal(tu, tu_c) and torch.equal(pm, pm_c) and torch.equal(st, st_c)
    assert torch.equal(l2, lvl) and torch.equal(r2, rec)
    y0 = buf[:W * H].reshape(H, W)
    want = T.rd_plane(y0, 32, 27, 200, True)
    assert np.array_equal(tu_y.cpu().numpy()[0], want[0]) and np.array_equal(st_y.cpu().numpy()[0], want[4])
    v1 = buf[fe + W * H + (W // 2) * (H // 2):2 * fe].reshape(H // 2, W // 2)
    want = T.rd_plane(v1, 16, 27, 200, False)
    assert np.array_equal(tu_c.cpu().numpy()[3], want[0]) and np.array_equal(st_c.cpu().numpy()[3], want[4])
    assert np.array_equal(rec.cpu().numpy()[2 * fe - v1.size:].reshape(v1.shape), want[3])


def test_single_plane_form(torch, gpu):
    src = T.mixed_picture(36, 44)
    lvl, rec, tu, pm, stats = gpu.tu_rd_plane(torch.from_numpy(src).cuda(), 16, 22, 400, False)
    want = T.rd_plane(src, 16, 22, 400, False)
    for a, b in zip((tu, pm, lvl, rec, stats), want):
        assert np.array_equal(a.cpu().numpy(), b)


def test_plumbing(torch, gpu):
    h, w = 32, 32
    ps = gpu.plane_set(0, w, h, w)
    src = torch.from_numpy(noisy8(h, w, 1).ravel().copy()).cuda()
    n, u = h * w, (h // 4) * (w // 4)
    ok = dict(lvl=torch.zeros(n, dtype=torch.int32, device="cuda"), rec=torch.zeros(n, dtype=torch.int16, device="cuda"),
              tu=torch.zeros(u, dtype=torch.uint8, device="cuda"), pm=torch.zeros(u, dtype=torch.uint8, device="cuda"))
    out = gpu.tu_rd_planes(src, ps, 32, 30, 5, True, **ok)
    assert all(out[i] is ok[k] for i, k in enumerate(("lvl", "rec", "tu", "pm")))
    wrong = [("lvl", torch.zeros(n, dtype=torch.int16, device="cuda"), TypeError),
             ("rec", torch.zeros(n, dtype=torch.int32, device="cuda"), TypeError),
             ("tu", torch.zeros(u, dtype=torch.int8, device="cuda"), TypeError),
             ("pm", torch.zeros(u, dtype=torch.int32, device="cuda"), TypeError),
             ("lvl", torch.zeros(n, dtype=torch.int32), TypeError),
             ("pm", torch.zeros(u, dtype=torch.uint8), TypeError),
             ("lvl", torch.zeros(n - 1, dtype=torch.int32, device="cuda"), ValueError),
             ("rec", torch.zeros(n - 1, dtype=torch.int16, device="cuda"), ValueError),
             ("tu", torch.zeros(u - 1, dtype=torch.uint8, device="cuda"), ValueError),
             ("pm", torch.zeros((1, 4, 16), dtype=torch.uint8, device="cuda"), ValueError)]
    for key, t, exc in wrong:
        with pytest.raises(exc):
            gpu.tu_rd_planes(src, ps, 32, 30, 5, True, **dict(ok, **{key: t}))
        if key != "tu":
            with pytest.raises(exc):
                gpu.tu_encode_map_planes(src, out[2], ps, 32, 30, 5, True,
                                         **{k: v for k, v in dict(ok, **{key: t}).items() if k != "tu"})
    with pytest.raises(ValueError):
        gpu.tu_encode_map_planes(src, torch.zeros(u - 1, dtype=torch.uint8, device="cuda"), ps, 32)
    for bad in (dict(ctb=8), dict(qp=52), dict(qp=-1), dict(lam=-1), dict(lam=2 ** 31)):
        with pytest.raises(ValueError):
            gpu.tu_rd_planes(src, ps, **dict(dict(ctb=32, qp=30, lam=0), **bad))
    with pytest.raises(ValueError):
        gpu.tu_rd_planes(src, gpu.plane_set(0, 30, 32, 32), 32)
    with pytest.raises(ValueError):
        gpu.tu_rd_planes(src, gpu.plane_set(4, w, h, w), 32)   # reaches outside the buffer
    # stats are overwritten by every call, never accumulated
    a = gpu.tu_rd_planes(src, ps, 32, 30, 5, True, **ok)[4].cpu().numpy()
    b = gpu.tu_rd_planes(src, ps, 32, 30, 5, True, **ok)[4].cpu().numpy()
    assert np.array_equal(a, b) and a[0, 0] == a[0, 1] + 5 * a[0, 2]
