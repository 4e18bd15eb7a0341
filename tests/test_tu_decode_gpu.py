"""GPU parity of the config-4 closed-loop decoder:
``gpu.tu_pred_map_closed``, ``gpu.dequant_inv_tu``, ``gpu.tu_decode_closed`` and
``gpu.tu_decode_closed_yuv420`` against the pinned oracle (tests/tu_decode_ref.py),
the GPU encoder's own reconstruction and the reference's recorded outputs.
Bar: bit-exact everywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tu_decode_ref as R  # noqa: E402

SENTINEL = -12345
SEED = 2024


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


def _content(kind, rng, h, w):
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 70 * np.sin(xx / 11.0) + 45 * np.cos(yy / 7.0)
        return np.clip(base + rng.normal(0, 3, (h, w)), 0, 255).astype(np.int16)
    if kind == "noise8":
        return rng.integers(0, 256, (h, w)).astype(np.int16)
    assert kind == "int16"
    return rng.integers(-32768, 32768, (h, w)).astype(np.int16)


def _planes(pset):
    """(plane index, element offset) of every plane of a set."""
    for g in range(pset.num_groups):
        for c in range(pset.planes_per_group):
            yield g * pset.planes_per_group + c, pset.base + g * pset.group_stride + c * pset.plane_stride


def _view(buf, pset, off):
    return np.lib.stride_tricks.as_strided(buf[off:], (pset.height, pset.width),
                                           (pset.pitch * buf.itemsize, buf.itemsize))


def _outside_mask(n, pset):
    m = np.ones(n, bool)
    for _, off in _planes(pset):
        _view(m, pset, off)[:] = False
    return m


def _sizes(tu, ctb):
    return sorted({n for _, _, n in R.tus(tu, ctb)})


# ------------------------------------------------------------------ 0. recorded outputs

@pytest.mark.parametrize("tag", ["k4y", "k4u", "k4n"])
def test_recorded_closed4(torch, gpu, golden, tag):
    g = golden("closed4.npz")
    ctb, qp, luma = int(g[tag + "_ctb"]), int(g[tag + "_qp"]), bool(g[tag + "_luma"])
    src, rec, tu, lvl = g[tag + "_src"], g[tag + "_rec"], g[tag + "_tu"], g[tag + "_lvl"]
    h, w = src.shape
    ps = gpu.plane_set(0, w, h, w)
    d_tu = torch.from_numpy(np.ascontiguousarray(tu)).cuda()
    pm = gpu.tu_pred_map_closed(torch.from_numpy(src.ravel().copy()).cuda(), torch.from_numpy(rec.ravel().copy()).cuda(),
                                d_tu, ps, ctb)
    assert np.array_equal(pm.cpu().numpy()[0], R.pred_map(src, rec, tu, ctb))
    out = torch.full((h * w,), SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.tu_decode_closed(d_tu, pm, torch.from_numpy(lvl.ravel().copy()).cuda(), ps, ctb, qp, luma, rec=out)
    assert dec is out and np.array_equal(dec.cpu().numpy().reshape(h, w), rec)


# ------------------------------------------------------------------ 1. pred map vs CPU

PRED_CASES = {"luma": (64, 96, 32, 0, 1, True, [4, 8, 16, 32]), "chroma": (36, 68, 16, 1, 2, False, [4, 8, 16])}


@pytest.mark.parametrize("kind", ["smooth", "noise8", "int16"])
@pytest.mark.parametrize("case", ["luma", "chroma"])
def test_pred_map_matches_cpu(torch, gpu, case, kind):
    h, w, ctb, pid, ppg, luma, want_sizes = PRED_CASES[case]
    rng = np.random.default_rng(31 + len(kind) + h)
    src = np.concatenate([_content(kind, rng, h, w).ravel() for _ in range(ppg)])
    ps = gpu.plane_set(0, w, h, w, planes_per_group=ppg, num_groups=1, plane_stride=h * w)
    d_src = torch.from_numpy(src).cuda()
    lvl, rec, tu = gpu.tu_pipeline_closed(d_src, ps, ctb, pid, SEED, 22, luma)
    pm = torch.full(tu.shape, 7, dtype=torch.uint8, device="cuda")
    assert gpu.tu_pred_map_closed(d_src, rec, tu, ps, ctb, pm=pm) is pm
    pm, tu, rec = pm.cpu().numpy(), tu.cpu().numpy(), rec.cpu().numpy()
    sizes, values = set(), set()
    for pl, off in _planes(ps):
        assert R.valid(tu[pl], ctb)
        want = R.pred_map(_view(src, ps, off), _view(rec, ps, off), tu[pl], ctb)
        assert np.array_equal(pm[pl], want), (case, kind, pl)
        sizes |= set(_sizes(tu[pl], ctb))
        values |= set(np.unique(want).tolist())
    assert sorted(sizes) == want_sizes          # every TU size the CTB allows
    if kind != "noise8":
        assert values == {0, 1}                 # both choices occur


# ------------------------------------------------------------------ 2. stage R per size

def _uniform_map(h, w, v):
    return np.full((h // 4, w // 4), v, np.uint8)


def _stage_r(torch, gpu, lvl2d, tu, ctb, luma, qp, base=0, pitch=None):
    h, w = lvl2d.shape
    pitch = pitch or w
    ps = gpu.plane_set(base, w, h, pitch)
    buf = np.zeros(base + h * pitch + 5, lvl2d.dtype)
    _view(buf, ps, base)[:] = lvl2d
    out = torch.full(buf.shape, SENTINEL, dtype=torch.int16, device="cuda")
    r = gpu.dequant_inv_tu(torch.from_numpy(buf).cuda(), torch.from_numpy(tu).cuda(), ps, ctb, luma, qp, out=out)
    assert r is out
    out = out.cpu().numpy()
    assert (out[_outside_mask(out.size, ps)] == SENTINEL).all()
    return _view(out, ps, base).copy()


EXTREMES = np.array([-2 ** 31, 2 ** 31 - 1, 32768, -32768, 32767, -32767, 0], np.int64)


@pytest.mark.parametrize("luma,v", [(True, 2), (True, 3), (True, 4), (True, 5), (False, 2), (False, 3), (False, 4)])
def test_stage_r_per_size(torch, gpu, luma, v):
    h, w, ctb = 32, 64, 32 if luma else 16
    tu = _uniform_map(h, w, v)
    assert R.valid(tu, ctb)
    rng = np.random.default_rng(200 + v + 10 * luma)
    src = torch.from_numpy(_content("smooth", rng, h, w).ravel()).cuda()
    enc = gpu.tu_pipeline_closed(src, gpu.plane_set(0, w, h, w), ctb, 0 if luma else 1, SEED, 22, luma)[0]
    levels = {"encoder": enc.cpu().numpy().reshape(h, w).astype(np.int32),
              "int16": rng.integers(-32768, 32768, (h, w)).astype(np.int32),
              "extremes": rng.choice(EXTREMES, (h, w)).astype(np.int32)}
    assert levels["encoder"].any()
    for name, lvl in levels.items():
        for qp in (0, 5, 24, 40, 41, 51):
            want = R.residual(lvl, tu, ctb, qp, luma)
            got = _stage_r(torch, gpu, lvl, tu, ctb, luma, qp)
            assert got.dtype == np.int16 and np.array_equal(got, want), (name, qp)
            assert np.array_equal(_stage_r(torch, gpu, lvl, tu, ctb, luma, qp, base=3, pitch=w + 5), want), (name, qp)
            if name != "extremes":   # the same values as int16 input, both forms
                l16 = lvl.astype(np.int16)
                assert np.array_equal(l16, lvl)
                assert np.array_equal(_stage_r(torch, gpu, l16, tu, ctb, luma, qp), want), (name, qp)
                assert np.array_equal(_stage_r(torch, gpu, l16, tu, ctb, luma, qp, base=1, pitch=w + 3), want), (name, qp)
    if v == 2:   # the 4x4 DST and the 4x4 DCT are told apart by these inputs
        assert not np.array_equal(R.residual(levels["int16"], tu, ctb, 24, True),
                                  R.residual(levels["int16"], tu, ctb, 24, False))


# ------------------------------------------------------------------ 3. round trip

@pytest.mark.parametrize("W,H,qp", [(96, 64, 4), (96, 64, 22), (96, 64, 32), (96, 64, 51), (72, 40, 22)])
def test_round_trip_yuv420(torch, gpu, W, H, qp):
    F = 2 if W == 96 else 3   # 3 frames: 6 chroma planes, a full group of 4 planes per wave and a short one
    luma, chroma = gpu.yuv420_plane_sets(F, W, H)
    assert (chroma.width, chroma.height) == (W // 2, H // 2)
    rng = np.random.default_rng(50 + qp + W)
    fe = gpu.yuv420_frame_elems(W, H)
    src = np.concatenate([np.concatenate([_content("smooth", rng, H, W).ravel(),
                                          _content("smooth", rng, H // 2, W // 2).ravel(),
                                          _content("noise8", rng, H // 2, W // 2).ravel()]) for _ in range(F)])
    assert src.size == F * fe
    d_src = torch.from_numpy(src).cuda()
    lvl, rec, tu_y, tu_c = gpu.tu_pipeline_closed_yuv420(d_src, luma, chroma, SEED, qp)
    pm_y = gpu.tu_pred_map_closed(d_src, rec, tu_y, luma, 32)
    pm_c = gpu.tu_pred_map_closed(d_src, rec, tu_c, chroma, 16)
    out = torch.full(rec.shape, SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.tu_decode_closed_yuv420(tu_y, pm_y, tu_c, pm_c, lvl, luma, chroma, qp, rec=out)
    assert dec is out and torch.equal(dec, rec)
    # the same through the two single-set calls on a fresh buffer
    one = gpu.tu_decode_closed(tu_y, pm_y, lvl, luma, 32, qp, True)
    one = gpu.tu_decode_closed(tu_c, pm_c, lvl, chroma, 16, qp, False, rec=one)
    assert torch.equal(one, rec)
    if qp == 22:   # and against the CPU restatement, first frame's Y and U
        dec = dec.cpu().numpy()
        for ps, tu, pm, ctb, lm in ((luma, tu_y, pm_y, 32, True), (chroma, tu_c, pm_c, 16, False)):
            want = R.decode(tu[0].cpu().numpy(), pm[0].cpu().numpy(), _view(lvl.cpu().numpy(), ps, ps.base), ctb, qp, lm)
            assert np.array_equal(_view(dec, ps, ps.base), want)


# ------------------------------------------------------------------ 4. maps no seed makes

def _alternating_map(h, w, ctb):
    tu = np.zeros((h // 4, w // 4), np.uint8)
    top = {16: 4, 32: 5}[ctb]
    k = 0
    for cy in range(0, h, ctb):
        for cx in range(0, w, ctb):
            tu[cy // 4:(cy + ctb) // 4, cx // 4:(cx + ctb) // 4] = 2 + k % (top - 1)
            k += 1
    return tu


def _decode_gpu(torch, gpu, tu, pm, lvl, ctb, qp, luma):
    h, w = lvl.shape
    out = torch.full((h * w,), SENTINEL, dtype=torch.int16, device="cuda")
    gpu.tu_decode_closed(torch.from_numpy(tu).cuda(), torch.from_numpy(pm).cuda(),
                         torch.from_numpy(np.ascontiguousarray(lvl, np.int32).ravel()).cuda(),
                         gpu.plane_set(0, w, h, w), ctb, qp, luma, rec=out)
    return out.cpu().numpy().reshape(h, w)


@pytest.mark.parametrize("name,h,w,ctb,luma", [("all4", 64, 96, 32, True), ("all4", 40, 72, 32, True),
                                                ("all4", 36, 68, 16, False), ("all32", 64, 96, 32, True),
                                                ("all16", 32, 48, 16, False), ("alt", 64, 128, 32, True),
                                                ("alt", 32, 80, 16, False)])
def test_maps_no_seed_makes(torch, gpu, name, h, w, ctb, luma):
    tu = {"all4": lambda: _uniform_map(h, w, 2), "all16": lambda: _uniform_map(h, w, 4),
          "all32": lambda: _uniform_map(h, w, 5), "alt": lambda: _alternating_map(h, w, ctb)}[name]()
    assert R.valid(tu, ctb)
    if name == "alt":
        assert _sizes(tu, ctb) == ([4, 8, 16, 32] if ctb == 32 else [4, 8, 16])
    rng = np.random.default_rng(h + w + ctb)
    lvl = (rng.integers(-3, 4, (h, w)) * (rng.random((h, w)) < 0.5)).astype(np.int32)
    pm = np.zeros_like(tu)
    for x, y, n in R.tus(tu, ctb):   # one random choice per TU, on every unit of it
        pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = rng.integers(0, 2)
    want = R.decode(tu, pm, lvl, ctb, 27, luma)
    railed = float(((want == 0) | (want == 255)).mean())
    assert railed < 0.5 and len(np.unique(want)) > 50   # the clip cannot hide a wrong prediction or residual
    assert np.array_equal(_decode_gpu(torch, gpu, tu, pm, lvl, ctb, 27, luma), want)
    # the decoder reads a TU's mode at its top-left unit only
    noisy = rng.integers(0, 2, pm.shape).astype(np.uint8)
    for x, y, n in R.tus(tu, ctb):
        noisy[y // 4, x // 4] = pm[y // 4, x // 4]
    assert np.array_equal(_decode_gpu(torch, gpu, tu, noisy, lvl, ctb, 27, luma), want)


# ------------------------------------------------------------------ 5. int16 wrap

def test_int16_wrap(torch, gpu):
    h, w, ctb, qp = 64, 128, 32, 24
    tu = _alternating_map(h, w, ctb)
    rng = np.random.default_rng(77)
    lvl = rng.integers(-2, 3, (h, w)).astype(np.int32)
    pm = np.zeros_like(tu)
    big = 0
    for k, (x, y, n) in enumerate(R.tus(tu, ctb)):
        pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = k & 1
        if k % 3 == 0:   # a DC level whose residual is about 32,730: dequantised 40 l, residual 4 * 40 l / n^2
            lvl[y, x] = round(32730 * n * n / 160)
            big += int(R.residual_tu(lvl[y:y + n, x:x + n], qp, n == 4).max() >= 32700)
    assert big >= 4
    want = R.decode(tu, pm, lvl, ctb, qp, True)
    nowrap = R.decode(tu, pm, lvl, ctb, qp, True,
                      reconstruct=lambda p, r: np.clip(p.astype(np.int32) + r.astype(np.int32), 0, 255).astype(np.int16))
    assert not np.array_equal(want, nowrap)   # the input tells the wrapping add from a wide one
    assert np.array_equal(_decode_gpu(torch, gpu, tu, pm, lvl, ctb, qp, True), want)


# ------------------------------------------------------------------ 6. layout

@pytest.mark.parametrize("base,pitch,pstride,gpad", [(16, 96, 48, 32), (3, 87, 43, 5)])
def test_layout_pitch_base_side_by_side_gaps(torch, gpu, base, pitch, pstride, gpad):
    """Two planes side by side in the same rows (plane stride < pitch), a base offset, a gap
    after every group; the first layout takes the vector row pieces, the second the scalar form."""
    h, w, ctb, qp = 40, 40, 32, 30
    gs = h * pitch + gpad
    ps = gpu.plane_set(base, w, h, pitch, planes_per_group=2, num_groups=2, plane_stride=pstride, group_stride=gs)
    n = base + 2 * gs + 9
    rng = np.random.default_rng(base)
    src = rng.integers(0, 256, n).astype(np.int16)
    d_src = torch.from_numpy(src).cuda()
    lvl, rec, tu = gpu.tu_pipeline_closed(d_src, ps, ctb, 0, SEED, qp, True)
    pm = gpu.tu_pred_map_closed(d_src, rec, tu, ps, ctb)
    outside = _outside_mask(n, ps)
    assert outside.sum() > 100
    res = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
    gpu.dequant_inv_tu(lvl, tu, ps, ctb, True, qp, out=res)
    out = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
    gpu.tu_decode_closed(tu, pm, lvl, ps, ctb, qp, True, rec=out)
    out, res, rec, lvl_h = out.cpu().numpy(), res.cpu().numpy(), rec.cpu().numpy(), lvl.cpu().numpy()
    assert (out[outside] == SENTINEL).all() and (res[outside] == SENTINEL).all()
    tu, pm = tu.cpu().numpy(), pm.cpu().numpy()
    for pl, off in _planes(ps):
        assert np.array_equal(_view(out, ps, off), _view(rec, ps, off)), pl
        assert np.array_equal(pm[pl], R.pred_map(_view(src, ps, off), _view(rec, ps, off), tu[pl], ctb)), pl
        assert np.array_equal(_view(res, ps, off), R.residual(_view(lvl_h, ps, off), tu[pl], ctb, qp, True)), pl
    assert np.array_equal(_view(out, ps, base + gs + pstride),
                          R.decode(tu[3], pm[3], _view(lvl_h, ps, base + gs + pstride), ctb, qp, True))


# ------------------------------------------------------------------ 7. recycling

def test_more_ctu_rows_than_resident_waves(torch, gpu):
    """k_tu_dec_closed runs 64-thread workgroups, one wave each; the launch is capped at the
    occupancy query's workgroups per CU times the CUs.  A gfx950 SIMD holds at most 8 waves,
    a CU has 4 SIMDs and an MI355X 256 CUs: at most 8 * 4 * 256 = 8,192 waves are resident,
    whatever the kernel's register count allows (91 VGPRs at CTB 32: 5 per SIMD, 5,120).  16,384 CTU rows
    are therefore at least twice the resident waves: every wave takes further tickets after its
    first row, and rows wait on rows claimed by recycled waves."""
    h, w, ctb, qp, P = 64, 32, 32, 28, 8192
    assert P * (h // ctb) >= 2 * 8 * 4 * 256
    rng = np.random.default_rng(8)
    distinct = [_content(k, rng, h, w) for k in ("smooth", "noise8", "smooth", "noise8")]
    d4 = torch.from_numpy(np.stack(distinct).reshape(4, h * w)).cuda()
    d_src = d4.repeat(P // 4, 1).reshape(-1).contiguous()
    ps = gpu.plane_set(0, w, h, w, planes_per_group=1, num_groups=P, group_stride=h * w)
    lvl, rec, tu = gpu.tu_pipeline_closed(d_src, ps, ctb, 0, SEED, qp, True)
    pm = gpu.tu_pred_map_closed(d_src, rec, tu, ps, ctb)
    out = torch.full(rec.shape, SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.tu_decode_closed(tu, pm, lvl, ps, ctb, qp, True, rec=out)
    assert torch.equal(dec, rec)
    first = dec[:4 * h * w].cpu().numpy().reshape(4, h, w)
    tu4, pm4, lvl4 = tu[:4].cpu().numpy(), pm[:4].cpu().numpy(), lvl[:4 * h * w].cpu().numpy().reshape(4, h, w)
    for k in range(4):
        assert np.array_equal(first[k], R.decode(tu4[k], pm4[k], lvl4[k], ctb, qp, True)), k
    assert len({first[k].tobytes() for k in range(4)}) == 4


# ------------------------------------------------------------------ 8. bad input

def _bad_maps():
    four = lambda: _uniform_map(64, 64, 2)
    cases = {}
    for name, v in (("value 1", 1), ("value 6", 6)):
        m = four()
        m[7, 9] = v
        cases[name] = (m, None, 64, 32)
    cases["value 5 under CTB 16"] = (_uniform_map(64, 64, 5), None, 64, 16)
    lone = four()
    lone[2, 2] = 3
    cases["lone 8x8 unit"] = (lone, None, 64, 32)
    cases["TU crossing the plane edge"] = (_uniform_map(36, 36, 3), None, 36, 32)
    pm = np.zeros((16, 16), np.uint8)
    pm[15, 15] = 2
    cases["pm value 2"] = (four(), pm, 64, 32)
    return cases


@pytest.mark.parametrize("name", list(_bad_maps()))
def test_bad_maps_are_value_errors(torch, gpu, name):
    """k_tu_dec_closed reads the status word before it takes a ticket and returns when it is
    set; the validity pre-pass precedes it on the stream: a flagged map returns, it cannot wait."""
    from nano_hevc import _lib
    tu, pm, size, ctb = _bad_maps()[name]
    assert pm is not None or not R.valid(tu, ctb)
    pm = np.zeros_like(tu) if pm is None else pm
    lvl = torch.zeros(size * size, dtype=torch.int32, device="cuda")
    ps = gpu.plane_set(0, size, size, size)
    d_tu, d_pm = torch.from_numpy(tu).cuda(), torch.from_numpy(pm).cuda()
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(d_tu, d_pm, lvl, ps, ctb, 30, True)
    strm = torch.cuda.current_stream()
    _, work = gpu._tu_decode_launch(d_tu, d_pm, lvl, ps, ctb, True, 30, None, strm)
    status = C.c_int(-1)
    assert _lib.load().nh_intra_rdo_closed_status(work.data_ptr(), C.byref(status), C.c_void_p(strm.cuda_stream)) == 0
    assert status.value == 2
    # the good neighbour of the case decodes
    good_tu = _uniform_map(size, size, 2)
    rec = gpu.tu_decode_closed(torch.from_numpy(good_tu).cuda(), torch.zeros_like(d_pm), lvl, ps, ctb, 30, True)
    assert int(rec.min()) == 128 and int(rec.max()) == 128   # zero levels: DC of the 128 border everywhere


def test_python_argument_checks(torch, gpu):
    ps = gpu.plane_set(0, 64, 64, 64)
    tu = torch.full((1, 16, 16), 2, dtype=torch.uint8, device="cuda")
    pm = torch.zeros_like(tu)
    lvl = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        gpu.tu_decode_closed(tu, pm, lvl.short(), ps, 32)                    # lvl must be int32
    with pytest.raises(TypeError):
        gpu.tu_decode_closed(tu.int(), pm, lvl, ps, 32)                      # maps must be uint8
    with pytest.raises(TypeError):
        gpu.tu_decode_closed(tu.cpu(), pm, lvl, ps, 32)                      # and on the device
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu.reshape(-1)[:255], pm, lvl, ps, 32)          # too few units
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu.reshape(1, 8, 32), pm, lvl, ps, 32)          # wrong trailing shape
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu, pm, lvl[:4000], ps, 32)                     # the set reaches outside lvl
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu, pm, lvl, ps, 32, rec=torch.zeros(100, dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu, pm, lvl, ps, 8)                             # ctb
    with pytest.raises(ValueError):
        gpu.tu_decode_closed(tu, pm, lvl, gpu.plane_set(0, 62, 64, 64), 32)  # width not a multiple of 4
    with pytest.raises(TypeError):
        gpu.dequant_inv_tu(lvl.long(), tu, ps, 32)
    with pytest.raises(TypeError):
        gpu.tu_pred_map_closed(lvl, lvl.short(), tu, ps, 32)                 # src must be int16


def test_yuv420_bad_chroma_map_names_the_set(torch, gpu):
    """Both sets' status words travel in one round trip; a set bit is then traced to its set."""
    W, H = 64, 64
    luma, chroma = gpu.yuv420_plane_sets(1, W, H)
    lvl = torch.zeros(gpu.yuv420_frame_elems(W, H), dtype=torch.int32, device="cuda")
    tu_y = torch.full((1, 16, 16), 2, dtype=torch.uint8, device="cuda")
    tu_c = torch.full((2, 8, 8), 2, dtype=torch.uint8, device="cuda")
    pm_y, pm_c = torch.zeros_like(tu_y), torch.zeros_like(tu_c)
    rec = gpu.tu_decode_closed_yuv420(tu_y, pm_y, tu_c, pm_c, lvl, luma, chroma, 30)
    assert int(rec.min()) == 128 and int(rec.max()) == 128
    bad = tu_c.clone()
    bad[1, 3, 3] = 5   # a 32x32 TU under CTB 16
    with pytest.raises(ValueError, match="chroma"):
        gpu.tu_decode_closed_yuv420(tu_y, pm_y, bad, pm_c, lvl, luma, chroma, 30)
    with pytest.raises(ValueError, match="luma"):
        gpu.tu_decode_closed_yuv420(bad[1:2].repeat(1, 2, 2).contiguous(), pm_y, tu_c, pm_c, lvl, luma, chroma, 30)
