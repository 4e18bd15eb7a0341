"""GPU parity of the closed-loop intra decoder at N = 4 (DST and DCT), 16 and 32
(DESIGN.md §3.9a, §4.3e): stage R (``gpu.dequant_inv_n``) and
``gpu.intra_decode_closed_n`` against the pinned-oracle helper
tests/decode_n_ref.py, the reference's recorded cases
(tests/golden/rdo_closed_n.npz) and the encoder ``gpu.intra_rdo_closed_n`` whose
outputs it decodes.  Bar: bit-exact; every output buffer is filled with a sentinel
first.  No test provokes a stall."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import decode_n_ref as dn  # noqa: E402
import rdo_closed_ref as ref  # noqa: E402
import rdo_plant  # noqa: E402

SENTINEL = -12345
KINDS = list(dn.KINDS)


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


def _stage_r(torch, gpu, lvl, sets, n, qp, dst):
    out = torch.full(lvl.shape, SENTINEL, dtype=torch.int16, device="cuda")
    r = gpu.dequant_inv_n(torch.from_numpy(lvl).cuda(), sets, n, qp, dst, out=out)
    assert r is out
    return out.cpu().numpy()


def _decode_sets(torch, gpu, modes, lvl, sets, n, qp, dst, **kw):
    """The decoder over plane sets of the 1-D level buffer ``lvl``; rec pre-filled with SENTINEL."""
    rec = torch.full(lvl.shape, SENTINEL, dtype=torch.int16, device="cuda")
    got = gpu.intra_decode_closed_n(torch.from_numpy(np.array(modes, np.uint8).ravel()).cuda(),     # copies: the shared
                                    torch.from_numpy(np.array(lvl, np.int32)).cuda(), sets, n, qp, dst,   # inputs are read only
                                    rec=rec, **kw)
    assert got is rec
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _decode_plane(torch, gpu, modes, lvl, n, qp, dst):
    h, w = lvl.shape
    return _decode_sets(torch, gpu, modes, lvl.ravel(), [gpu.plane_set(0, w, h, w)], n, qp, dst).reshape(h, w)


def _expect_sets(modes, lvl, sets, n, qp, dst):
    """The helper over plane sets: recon with SENTINEL everywhere outside the plane rectangles."""
    rec = np.full(lvl.shape, SENTINEL, np.int16)
    mo = 0
    for lv, rv in zip(_plane_views(lvl, sets), _plane_views(rec, sets)):
        bh, bw = lv.shape[0] // n, lv.shape[1] // n
        rv[:] = dn.decode(modes[mo:mo + bh * bw].reshape(bh, bw), np.ascontiguousarray(lv), qp, n, dst)
        mo += bh * bw
    assert mo == modes.size
    return rec


def _same(got, want, what="rec"):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:4]}: " \
                          f"{got.ravel()[bad[:4]]} vs {want.ravel()[bad[:4]]}"


def _random_case(rng, h, w, n, amp=3):
    modes = rng.integers(0, 35, (h // n, w // n)).astype(np.uint8)
    lvl = rng.integers(-amp, amp + 1, (h, w)).astype(np.int32)
    return modes, lvl


def _amp(n):
    """Amplitude of the dense random levels of the layout tests (QP 27), per N."""
    return {4: 1, 16: 2, 32: 8}[n]


# ------------------------------------------------------------------ 1. the reference's recorded cases

@pytest.mark.parametrize("k", range(4))
def test_recorded_reference_cases(torch, gpu, golden, k):
    g = golden("rdo_closed_n.npz")
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    got = _decode_plane(torch, gpu, g[f"c{k}_modes"], g[f"c{k}_lvl"].astype(np.int32), n, qp, dst)
    _same(got, g[f"c{k}_rec"])


# ------------------------------------------------------------------ 2. every mode at every position class

@pytest.mark.parametrize("n,dst", KINDS)
def test_every_mode_at_every_position(torch, gpu, n, dst):
    modes, lvl, qp, want = dn.every_mode(n, dst)
    blocks, nonzero, constant, railed = dn.every_mode_census(n, dst)
    print(f"N = {n} dst = {dst}: {nonzero}/{blocks} nonzero residuals, {constant} constant blocks, "
          f"{100 * railed:.1f} % of the samples at 0 or 255")
    assert nonzero == blocks == 315 and constant == 0 and railed <= dn.RAILED_CAP
    h, w = dn.every_mode_shape(n)
    sets = [gpu.plane_set(0, w, h, w, 1, dn.EVERY_MODE_PLANES, 0, h * w)]
    got = _decode_sets(torch, gpu, modes, lvl.ravel(), sets, n, qp, dst)
    _same(got, want.ravel())


# ------------------------------------------------------------------ 3. stage R alone

@pytest.mark.parametrize("qp", [0, 5, 23, 24, 51, -3, 60])
@pytest.mark.parametrize("n,dst", KINDS)
def test_stage_r_full_range(torch, gpu, n, dst, qp):
    """Full-range levels of both dtypes on a ragged plane with an odd base and pitch (element accesses)."""
    h, w, base = 2 * n + 3, 3 * max(n, 16) + 1, 3
    pitch = w + 2
    full = (h // n) * (w // n) * n * n
    s = [gpu.plane_set(base, w, h, pitch)]
    for dtype in (np.int16, np.int32):
        rng = np.random.default_rng(1000 + 7 * n + dst + (500 if dtype is np.int32 else 0))
        lvl = _full_range(rng, base + h * pitch, dtype)
        want = np.full(lvl.shape, SENTINEL, np.int16)
        dn.residual_plane(next(_plane_views(lvl, s)), qp, next(_plane_views(want, s)), n, dst)
        assert len(np.unique(want)) > full // 2 and (want == SENTINEL).sum() >= lvl.size - full   # the outputs span int16
        _same(_stage_r(torch, gpu, lvl, s, n, qp, dst), want, f"res {dtype.__name__}")


@pytest.mark.parametrize("n,dst", KINDS)
def test_stage_r_forms_and_dtypes_agree(torch, gpu, n, dst):
    """The vector-row form (base, pitch multiples of 8) and the element form (odd base and pitch) on the
    same blocks, and int16 against int32 levels of int16 range."""
    rng = np.random.default_rng(50 + n + dst)
    h, w = 2 * n + 1, 2 * n + 5
    blocks = _full_range(rng, (h, w), np.int16)
    res = []
    for base, pitch in ((16, (w + 7) // 8 * 8 + 8), (3, w + 4)):
        s = [gpu.plane_set(base, w, h, pitch)]
        for dtype in (np.int16, np.int32):
            buf = np.zeros(base + h * pitch, dtype)
            next(_plane_views(buf, s))[:] = blocks
            out = _stage_r(torch, gpu, buf, s, n, 33, dst)
            res.append(next(_plane_views(out, s)).copy())
            assert (out == SENTINEL).sum() >= out.size - (h // n) * (w // n) * n * n
    want = np.full((h, w), SENTINEL, np.int16)
    dn.residual_plane(blocks, 33, want, n, dst)
    for r in res:
        _same(r, want, "res")


# ------------------------------------------------------------------ 4. the int16 wrap

@pytest.mark.parametrize("n,dst", KINDS)
def test_int16_wrap(torch, gpu, n, dst):
    modes, lvl, qp = dn.wrap_input(n, dst)
    wrap = dn.decode(modes, lvl, qp, n, dst)
    sat = dn.decode(modes, lvl, qp, n, dst, reconstruct=dn.saturating_reconstruct)
    assert int((wrap != sat).sum()) == dn.WRAP[(n, dst)][3] and (wrap[wrap != sat] == 0).all()
    _same(_decode_plane(torch, gpu, modes, lvl, n, qp, dst), wrap)


# ------------------------------------------------------------------ 5. narrowest shapes

@pytest.mark.parametrize("n,dst", KINDS)
def test_narrowest_shapes(torch, gpu, n, dst):
    for h, w in ((n, n), (n, 5 * n), (5 * n, n), (n - 1, n - 1)):
        rng = np.random.default_rng(100 * h + w)
        modes, lvl = _random_case(rng, h, w, n, _amp(n))
        got = _decode_plane(torch, gpu, modes, lvl, n, 27, dst)   # status 0: no exception
        _same(got, dn.decode(modes, lvl, 27, n, dst), f"rec {h}x{w}")
        if h < n:
            assert not got.any()


# ------------------------------------------------------------------ 6. layouts

@pytest.mark.parametrize("n,dst", KINDS)
def test_layouts_and_both_store_forms(torch, gpu, n, dst):
    """Pitch != width, a base offset, two planes side by side per group x two groups with gaps, and a
    half-size second set in the same call.  Once with bases, pitches and strides multiples of 8 (vector
    accesses) and once with an odd base (element accesses): each equals the helper.  Every element
    outside the plane rectangles keeps the sentinel."""
    w, h = 2 * n + 3, 2 * n + 2                      # 2 x 2 full blocks, ragged both ways
    pitch = (2 * w + 8 + 7) // 8 * 8                 # two planes side by side in a row, and a gap
    pstride = (w + 7) // 8 * 8
    gstride = h * pitch + 16
    w2, h2 = n + n // 2, n + 1                       # the half-size set: 1 x 1 full block
    outs = []
    for base in (8, 5):
        s1 = gpu.plane_set(base, w, h, pitch, 2, 2, pstride, gstride)
        base2 = (base + 2 * gstride + 8 + 7) // 8 * 8 + (base & 7)
        pitch2 = (w2 + 7) // 8 * 8 + 8
        s2 = gpu.plane_set(base2, w2, h2, pitch2, 1, 3, 0, h2 * pitch2 + 8)
        sets = [s1, s2]
        total = base2 + 3 * (h2 * pitch2 + 8) + 3
        rng = np.random.default_rng(600 + n)
        modes = rng.integers(0, 35, 4 * 4 + 3).astype(np.uint8)
        planes = [rng.integers(-_amp(n), _amp(n) + 1, shape) for shape in [(h, w)] * 4 + [(h2, w2)] * 3]
        lvl = rng.integers(-_amp(n), _amp(n) + 1, total).astype(np.int32)      # noise everywhere, gaps included
        for v, p in zip(_plane_views(lvl, sets), planes):                      # the same planes in both layouts
            v[:] = p
        got, want = _decode_sets(torch, gpu, modes, lvl, sets, n, 27, dst), _expect_sets(modes, lvl, sets, n, 27, dst)
        _same(got, want)
        assert (want == SENTINEL).sum() == total - 4 * w * h - 3 * w2 * h2
        outs.append([v.copy() for v in _plane_views(got, sets)])
    for a, b in zip(*outs):
        _same(a, b, "plane")


def test_eight_sets_of_0_to_3_block_rows(torch, gpu):
    n = 16
    # (h, w, planes per group, groups); set 2 is narrower than a block, set 5 has no group
    shapes = [(16, 33, 1, 1), (50, 17, 1, 2), (40, 15, 1, 1), (15, 40, 1, 1), (33, 32, 2, 1), (20, 20, 1, 0),
              (48, 16, 1, 1), (17, 49, 1, 1)]
    sets, off = [], 3
    for h, w, ppg, ng in shapes:
        sets.append(gpu.plane_set(off, w, h, w, ppg, ng, h * w + 2, ppg * (h * w + 2) + 1))
        off += max(1, ng) * (ppg * (h * w + 2) + 1) + 5
    rng = np.random.default_rng(77)
    lvl = rng.integers(-2, 3, off).astype(np.int32)
    nmodes = 2 + 2 * 3 + 0 + 0 + 2 * 4 + 0 + 3 + 3
    modes = rng.integers(0, 35, nmodes).astype(np.uint8)
    _same(_decode_sets(torch, gpu, modes, lvl, sets, n, 27, False), _expect_sets(modes, lvl, sets, n, 27, False))


# ------------------------------------------------------------------ 8. tickets recycle

@pytest.mark.parametrize("n,dst,planes", [(4, True, 8192), (16, False, 8192), (32, False, 4096)])
def test_more_rows_than_resident_workers(torch, gpu, n, dst, planes):
    """3 x ``planes`` block rows, at least 3x the one-wave workgroups the device can hold: 32 per CU x 256
    CUs = 8,192 at N = 4 (38 VGPRs, 8 waves per SIMD) and at most that at N = 16 (51 VGPRs, 104 SGPRs: 7
    waves per SIMD, 7,168), 16 per CU = 4,096 at N = 32 (118 VGPRs, 4 waves per SIMD) -- every worker
    claims further tickets.  The planes cycle through 4 (modes, levels) pairs; each plane must equal
    its pair's decode."""
    h, w = 3 * n, 2 * n
    rng = np.random.default_rng(1300 + n)
    pairs = [_random_case(rng, h, w, n, _amp(n)) for _ in range(4)]
    want = [dn.decode(m, l, 27, n, dst).ravel() for m, l in pairs]
    assert len({x.tobytes() for x in want}) == 4
    modes = np.concatenate([m.ravel() for m, _ in pairs] * (planes // 4))
    lvl = np.concatenate([l.ravel() for _, l in pairs] * (planes // 4))
    got = _decode_sets(torch, gpu, modes, lvl, [gpu.plane_set(0, w, h, w, 1, planes, 0, h * w)], n, 27, dst)
    got = got.reshape(planes // 4, 4, -1)
    for p in range(4):
        bad = np.flatnonzero((got[:, p] != want[p]).any(axis=1))
        assert bad.size == 0, f"{bad.size} planes of pair {p} differ, first {4 * bad[:4] + p}"


# ------------------------------------------------------------------ 9. round trip on the device

def _round_trip(torch, gpu, src, sets, n, qp, dst):
    d = torch.from_numpy(src).cuda()
    modes, lvl, rec, _ = gpu.intra_rdo_closed_n(d, sets, n, qp, dst)
    out = torch.full(src.shape, SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.intra_decode_closed_n(modes, lvl, sets, n, qp, dst, rec=out)
    torch.cuda.synchronize()
    assert torch.equal(dec, rec)
    return modes.cpu().numpy(), lvl.cpu().numpy(), dec.cpu().numpy()


@pytest.mark.parametrize("pad", [0, 13])
@pytest.mark.parametrize("n,dst", KINDS)
def test_round_trip_yuv420(torch, gpu, n, dst, pad):
    """The encoder's outputs decode to the encoder's recon; the first Y plane also against the helper."""
    W, H, F = 4 * n + 8, 2 * n + 4, 2
    qp = 4 if n == 32 else 22
    fs = gpu.yuv420_frame_elems(W, H) + pad
    sets = gpu.yuv420_plane_sets(F, W, H, frame_stride=fs if pad else None)
    assert len(sets) == 2 and (sets[1].width, sets[1].height) == (W // 2, H // 2)
    src = np.zeros(F * fs, np.int16)
    pic = ref.wide_picture if n == 32 else ref.picture
    for k, v in enumerate(_plane_views(src, sets)):
        v[:] = pic(*v.shape, 40 + k + n)
    if pad:   # an uncoded gap between frames: the encoder's recon buffer is zero there, the decoder's keeps
        src_gap = np.ones(src.shape, bool)   # its sentinel; compare the planes only
        for v in _plane_views(src_gap, sets):
            v[:] = False
    d = torch.from_numpy(src).cuda()
    modes, lvl, rec, _ = gpu.intra_rdo_closed_n(d, sets, n, qp, dst)
    out = torch.full(src.shape, SENTINEL, dtype=torch.int16, device="cuda")
    dec = gpu.intra_decode_closed_n(modes, lvl, sets, n, qp, dst, rec=out)
    torch.cuda.synchronize()
    dec, rec = dec.cpu().numpy(), rec.cpu().numpy()
    for a, b in zip(_plane_views(dec, sets), _plane_views(rec, sets)):
        _same(a, b, "plane")
    if pad:
        assert (dec[src_gap] == SENTINEL).all()
    y_modes = modes.cpu().numpy()[:(H // n) * (W // n)].reshape(H // n, W // n)
    y_lvl = lvl.cpu().numpy()[:W * H].reshape(H, W)
    assert len(np.unique(y_modes)) >= 3 and np.count_nonzero(y_lvl)
    _same(dec[:W * H].reshape(H, W), dn.decode(y_modes, y_lvl, qp, n, dst), "Y plane")


@functools.lru_cache(maxsize=None)
def _census_recipe(n, dst):
    """The first closed-loop noise recipe of rdo_plant.CENSUS for the kind: (amplitude, QP)."""
    return next((amp, qp) for (cn, cd, closed, amp, qp) in rdo_plant.CENSUS if (cn, cd, closed) == (n, dst, True))


@pytest.mark.parametrize("n,dst", KINDS)
def test_round_trip_noise_census(torch, gpu, n, dst):
    """All 35 modes come out of a real encoder (rdo_plant's census plane) and decode to its recon."""
    amp, qp = _census_recipe(n, dst)
    src = rdo_plant.census_plane(n, dst, amp)
    h, w = src.shape
    modes, lvl, _ = _round_trip(torch, gpu, np.ascontiguousarray(src).ravel(), [gpu.plane_set(0, w, h, w)], n, qp, dst)
    coded = np.abs(lvl.reshape(h // n, n, w // n, n)).max(axis=(1, 3)) > 0
    assert sorted(np.unique(modes.reshape(h // n, w // n)[coded]).tolist()) == list(range(35))


# ------------------------------------------------------------------ 10. errors and plumbing

def test_bad_mode_is_value_error(torch, gpu):
    n, h, w = 16, 96, 128
    rng = np.random.default_rng(9)
    modes, lvl = _random_case(rng, h, w, n, 2)
    bad = modes.copy()
    bad[4, 5] = 35
    with pytest.raises(ValueError, match="mode above 34"):
        _decode_plane(torch, gpu, bad, lvl, n, 30, False)
    _same(_decode_plane(torch, gpu, modes, lvl, n, 30, False), dn.decode(modes, lvl, 30, n, False))


def test_bad_arguments(torch, gpu):
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    lvl = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    modes = torch.zeros(16 * 16, dtype=torch.uint8, device="cuda")
    s = [gpu.plane_set(0, 64, 64)]
    with pytest.raises(ValueError, match="block_size"):
        gpu.intra_decode_closed_n(modes, lvl, s, 12, 30)
    with pytest.raises(ValueError, match="block_size"):
        gpu.dequant_inv_n(lvl, s, 12, 30)
    with pytest.raises(ValueError, match="use_dst"):
        gpu.intra_decode_closed_n(modes, lvl, s, 16, 30, use_dst=True)
    with pytest.raises(ValueError, match="use_dst"):
        gpu.dequant_inv_n(lvl, s, 16, 30, use_dst=True)
    for sets in ([], s * 9):
        with pytest.raises(ValueError, match="nsets"):
            gpu.intra_decode_closed_n(modes, lvl, sets, 16, 30)
        with pytest.raises(ValueError, match="nsets"):
            gpu.dequant_inv_n(lvl, sets, 16, 30)
    with pytest.raises(ValueError, match="15 modes for 16 blocks"):
        gpu.intra_decode_closed_n(modes[:15], lvl, s, 16, 30)
    L = _lib.load()
    out = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    ps = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    assert L.nh_dequant_inv_planes_n(lvl.data_ptr(), 3, out.data_ptr(), C.byref(ps), 1, 16, 0, 30, None) == _lib.NH_EARG
    assert b"lvl_bytes" in L.nh_last_error()


@pytest.mark.parametrize("n,dst", KINDS)
def test_qp_is_clamped(torch, gpu, n, dst):
    rng = np.random.default_rng(60 + n)
    modes, lvl = _random_case(rng, 2 * n + 1, 2 * n + 2, n, 1)
    lvl = (lvl * (rng.random(lvl.shape) < 0.1)).astype(np.int32)
    for qp, like in ((-3, 0), (60, 51)):
        got = _decode_plane(torch, gpu, modes, lvl, n, qp, dst)
        _same(got, _decode_plane(torch, gpu, modes, lvl, n, like, dst), f"rec at QP {qp}")
        _same(got, dn.decode(modes, lvl, like, n, dst), f"rec at QP {qp}")
    assert not np.array_equal(dn.decode(modes, lvl, 0, n, dst), dn.decode(modes, lvl, 51, n, dst))


def test_block_size_8_is_the_existing_decoder(torch, gpu):
    rng = np.random.default_rng(8)
    sets = [gpu.plane_set(0, 40, 24, 40, 1, 2, 0, 24 * 40 + 24 * 20), gpu.plane_set(24 * 40, 20, 12, 20, 2, 2, 240,
                                                                                     24 * 40 + 24 * 20)]
    lvl = torch.from_numpy(rng.integers(-3, 4, 2 * (24 * 40 + 24 * 20)).astype(np.int32)).cuda()
    modes = torch.from_numpy(rng.integers(0, 35, 2 * 15 + 4 * 2).astype(np.uint8)).cuda()
    a = gpu.intra_decode_closed_n(modes, lvl, sets, 8, 27)
    b = gpu.intra_decode_closed(modes, lvl, sets, 27)
    ra = gpu.dequant_inv_n(lvl, sets, 8, 27)
    rb = gpu.dequant_inv8x8(lvl, sets, 27)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ra, rb) and len(torch.unique(a)) > 50


def test_caller_buffer_and_stream(torch, gpu):
    n, h, w = 16, 45, 75
    rng = np.random.default_rng(12)
    modes, lvl = _random_case(rng, h, w, n, 2)
    want = dn.decode(modes, lvl, 25, n, False)
    d_modes, d_lvl = torch.from_numpy(modes.ravel()).cuda(), torch.from_numpy(lvl).cuda()
    s = [gpu.plane_set(0, w, h, w)]
    fresh = gpu.intra_decode_closed_n(d_modes, d_lvl, s, n, 25)
    torch.cuda.synchronize()
    _same(fresh.cpu().numpy(), want)
    rec = torch.full((h, w), SENTINEL, dtype=torch.int16, device="cuda")
    res = torch.full((h, w), SENTINEL, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()   # the inputs are ready before the side stream reads them
    side = torch.cuda.Stream()
    got = gpu.intra_decode_closed_n(d_modes, d_lvl, s, n, 25, rec=rec, stream=side)
    r = gpu.dequant_inv_n(d_lvl, s, n, 25, out=res, stream=side)
    side.synchronize()
    assert got is rec and r is res
    _same(got.cpu().numpy(), want)
    _same(r.cpu().numpy(), dn.residual_plane(lvl, 25, np.full((h, w), SENTINEL, np.int16), n))
