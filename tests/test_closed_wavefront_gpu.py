"""GPU parity of the two closed-loop row wavefronts of config 3 where the rest of
the suite does not reach: the encoder
``gpu.intra_rdo_closed`` (k_intra_rdo8_closed_tag, packed and 32-bit forms) and
the decoder ``gpu.intra_decode_closed`` (k_intra_dec8_closed) with

a. more block rows than waves can be resident, so every wave takes several tickets;
b. pitch != width, planes side by side, gaps between groups and a base offset;
c. residuals that make the decoder's int16 ``pred + res`` wrap;
d. eight plane sets of mixed heights (closed_ticket's order-1 search).

References: tests/decode_ref.py (``decode``, ``residual_block``) and the pinned
oracle's ``intra_rdo_plane(..., closed=True)``, never the GPU.  Every buffer the
device writes starts as SENTINEL.  Bar: bit-exact.  The ticket map itself is
walked on the host by test_closed_ticket_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402  (checker only)
from decode_ref import decode, residual_block  # noqa: E402

SENTINEL = -12345
K = 32   # distinct payload planes per set of the recycling call


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
    """Writable (h, w) views of every plane of ``sets`` inside the 1-D array ``buf``, set by set,
    plane g * planes_per_group + c of a set: the order of the encoder's modes and SSEs."""
    for s in sets:
        for g in range(s.num_groups):
            for c in range(s.planes_per_group):
                b = s.base + g * s.group_stride + c * s.plane_stride
                yield np.lib.stride_tricks.as_strided(buf[b:], (s.height, s.width),
                                                      (s.pitch * buf.itemsize, buf.itemsize))


def _inside(n, sets):
    """True for the elements of an n-element buffer that lie inside a plane rectangle."""
    m = np.zeros(n, bool)
    for v in _plane_views(m, sets):
        v[:] = True
    return m


def _full(a):
    """The part of a plane that full 8x8 blocks cover."""
    return a[:a.shape[0] // 8 * 8, :a.shape[1] // 8 * 8]


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got != want)
    if bad.size:
        pytest.fail(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: "
                    f"got {got[bad[0]]}, want {want[bad[0]]}", pytrace=False)


def _levels(rng, shape, amp=3, dens=1.0):
    """The level generator of test_decode_every_mode_every_position."""
    return (rng.integers(-amp, amp + 1, shape) * (rng.random(shape) < dens)).astype(np.int32)


def _decode_gpu(torch, gpu, modes, lvl, sets, qp):
    """intra_decode_closed into a sentinel-filled rec; it returns only with device status 0
    (status 1, a stalled wavefront, raises RuntimeError; status 2 ValueError)."""
    rec = torch.full((lvl.size,), SENTINEL, dtype=torch.int16, device="cuda")
    got = gpu.intra_decode_closed(torch.from_numpy(modes).cuda(), torch.from_numpy(lvl).cuda(), sets, qp, rec=rec)
    assert got is rec
    return got.cpu().numpy()


def _encode_gpu(torch, gpu, src, sets, qp):
    """intra_rdo_closed into sentinel-filled lvl and rec; it returns only with device status 0."""
    lvl = torch.full((src.size,), SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full((src.size,), SENTINEL, dtype=torch.int16, device="cuda")
    m, l, r, s = gpu.intra_rdo_closed(torch.from_numpy(src).cuda(), sets, qp, lvl=lvl, rec=rec)
    assert l is lvl and r is rec
    return m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()


# ------------------------------------------------------------------ a. ticket recycling
#
# A wave that finishes a row takes the next ticket; the grid is min(rows, resident cap).
# The cap is occupancy x CUs, at most 32 waves/CU x 256 CUs = 8192 waves on an MI355X
# (the encoder's 32-bit form: a fixed 2048).  One call with
#   set 0: 8192 planes of 16 x 24 (2 x 3 blocks), two per group
#   set 1: 4096 planes of 40 x 8  (5 x 1 blocks)
# has 8192 * 3 + 4096 = 28,672 block rows = 3.5 x 8192 (14 x 2048), 4,456,448 samples:
# whatever occupancy the runtime reports, every resident wave takes several tickets, and
# line words are published and polled by waves on their second and later rows.  The
# planes are K = 32 distinct payloads per set, assigned by a seeded draw, so neighbouring
# planes differ and a row decoded into or from the wrong plane shows.

RECYCLE_SHAPES = ((24, 16), (8, 40))   # (h, w) per set
RECYCLE_PLANES = (8192, 4096)
RECYCLE_QP = 30   # the encoder tests'


@pytest.fixture(scope="module")
def recycle(gpu):
    n0 = RECYCLE_PLANES[0] * 24 * 16
    sets = [gpu.plane_set(0, 16, 24, 16, planes_per_group=2, num_groups=RECYCLE_PLANES[0] // 2,
                          plane_stride=24 * 16, group_stride=2 * 24 * 16),
            gpu.plane_set(n0, 40, 8, 40, planes_per_group=1, num_groups=RECYCLE_PLANES[1], group_stride=8 * 40)]
    rows = sum(s.height // 8 * s.planes_per_group * s.num_groups for s in sets)
    assert rows == 28672 and rows > 3 * 32 * 256
    pick = [np.random.default_rng(2024 + k).integers(0, K, p) for k, p in enumerate(RECYCLE_PLANES)]
    assert all(len(np.unique(p)) == K for p in pick)          # every payload is used
    assert all((p[1:] != p[:-1]).mean() > 0.9 for p in pick)  # neighbouring planes differ
    return sets, n0 + RECYCLE_PLANES[1] * 8 * 40, pick


def _assemble(payloads, pick):
    """Per-set payload arrays (K, ...) -> the call's buffer: plane p of set k is payloads[k][pick[k][p]]."""
    return np.concatenate([np.ascontiguousarray(a[p]).reshape(-1) for a, p in zip(payloads, pick)])


def test_recycle_decoder(torch, gpu, recycle):
    """28,672 block rows (3.5 x the 32 x 256 = 8192 waves an MI355X can hold): the decoder's
    waves each take several tickets.  Random modes 0..34, levels of the (QP 23, amp 3, dens 1.0)
    generator; every plane equals ``decode`` of its payload."""
    sets, n, pick = recycle
    qp, rng = 23, np.random.default_rng(31)
    modes, lvl, rec = [], [], []
    for h, w in RECYCLE_SHAPES:
        m = rng.integers(0, 35, (K, h // 8, w // 8)).astype(np.uint8)
        lv = _levels(rng, (K, h, w))
        r = np.stack([decode(m[k], lv[k], qp) for k in range(K)])
        assert len({x.tobytes() for x in r}) == K   # all 32 reconstructions are distinct
        modes.append(m)
        lvl.append(lv)
        rec.append(r)
    want = _assemble(rec, pick)
    assert want.size == n
    railed = float(((want == 0) | (want == 255)).mean())   # every sample is inside a full block here
    print(f"{100 * railed:.1f} % of the expected samples are 0 or 255")
    assert railed < 0.35   # the clip cannot hide a wrong prediction or residual
    got = _decode_gpu(torch, gpu, _assemble(modes, pick), _assemble(lvl, pick), sets, qp)
    _same(got, want, "recon")


@pytest.fixture(scope="module")
def recycle_sources():
    """K random 8-bit source planes per set with the oracle's closed-loop results."""
    rng = np.random.default_rng(47)
    src = [rng.integers(0, 256, (K, h, w)).astype(np.int16) for h, w in RECYCLE_SHAPES]
    return src, [_oracle_payloads(s, RECYCLE_QP) for s in src]


def _oracle_payloads(src, qp):
    res = [O.intra_rdo_plane(p, qp, closed=True) for p in src]
    return [np.stack([r[k] for r in res]) for k in range(3)] + [np.array([r[3] for r in res], np.int64)]


def _check_recycle_encoder(torch, gpu, recycle, src, ref):
    sets, n, pick = recycle
    m, l, r, s = _encode_gpu(torch, gpu, _assemble(src, pick), sets, RECYCLE_QP)
    for k, (got, name) in enumerate(((m, "modes"), (l, "levels"), (r, "recon"), (s, "sse"))):
        _same(got, _assemble([ref[0][k], ref[1][k]], pick), name)   # every sample is inside a full block


def test_recycle_encoder_packed(torch, gpu, recycle, recycle_sources):
    """The same 28,672 rows through the encoder's packed form (grid: occupancy x CUs <= 8192):
    modes, levels, recon and per-plane SSE against the oracle's closed loop."""
    src, ref = recycle_sources
    assert all(0 <= s.min() and s.max() <= 255 for s in src)
    _check_recycle_encoder(torch, gpu, recycle, src, ref)


def test_recycle_encoder_32bit(torch, gpu, recycle, recycle_sources):
    """One payload of set 0 holds a sample of 300, so the whole call takes the 32-bit form:
    2048 waves, 14 tickets each."""
    src, ref = recycle_sources
    src = [src[0].copy(), src[1]]
    src[0][5, 3, 7] = 300
    assert (recycle[2][0] == 5).any()
    ref0 = [a.copy() for a in ref[0]]
    for a, v in zip(ref0, O.intra_rdo_plane(src[0][5], RECYCLE_QP, closed=True)):
        a[5] = v
    _check_recycle_encoder(torch, gpu, recycle, src, [ref0, ref[1]])


# ------------------------------------------------------------------ b, d. layouts and many sets

def _check_decoder(torch, gpu, sets, n, qp, seed):
    """Decoder over ``sets`` inside an n-element buffer.  Levels outside full blocks (and outside the
    planes) are full-range garbage: nothing may read them."""
    rng = np.random.default_rng(seed)
    lvl = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    want = np.full(n, SENTINEL, np.int16)
    modes = [np.zeros(0, np.uint8)]
    for lv, wv in zip(_plane_views(lvl, sets), _plane_views(want, sets)):
        _full(lv)[:] = _levels(rng, _full(lv).shape)
        m = rng.integers(0, 35, (lv.shape[0] // 8, lv.shape[1] // 8)).astype(np.uint8)
        modes.append(m.ravel())
        wv[:] = decode(m, lv, qp)
    got = _decode_gpu(torch, gpu, np.concatenate(modes), lvl, sets, qp)
    for k, (g, wv) in enumerate(zip(_plane_views(got, sets), _plane_views(want, sets))):
        _same(_full(g), _full(wv), f"recon of plane {k}")
        h8, w8 = _full(g).shape
        assert not g[h8:].any() and not g[:, w8:].any(), f"plane {k}: recon outside full blocks is not 0"
    outside = ~_inside(n, sets)
    assert outside.any() and (got[outside] == SENTINEL).all(), "a write outside the plane rectangles"


def _check_encoder(torch, gpu, sets, n, qp, seed, wide=False):
    """Encoder over ``sets``.  Source elements outside the plane rectangles hold -7777: nothing may
    read them (not even the 8-bit test that picks the form)."""
    rng = np.random.default_rng(seed)
    src = np.full(n, -7777, np.int16)
    for v in _plane_views(src, sets):
        v[:] = rng.integers(0, 256, v.shape)
    if wide:   # one 9-bit sample in one plane: the whole call takes the 32-bit form
        v = list(_plane_views(src, sets))[4]
        assert v.shape[0] >= 8 and v.shape[1] >= 8
        v[2, 3] = 300
    ref = [O.intra_rdo_plane(v, qp, closed=True) for v in _plane_views(src, sets)]
    m, l, r, s = _encode_gpu(torch, gpu, src, sets, qp)
    _same(m, np.concatenate([np.zeros(0, np.uint8)] + [x[0].ravel() for x in ref]), "modes")
    _same(s, np.array([x[3] for x in ref], np.int64), "sse")
    for k, (gl, gr, x) in enumerate(zip(_plane_views(l, sets), _plane_views(r, sets), ref)):
        _same(_full(gl), _full(x[1]), f"levels of plane {k}")   # in-plane levels outside full blocks: unspecified
        _same(_full(gr), _full(x[2]), f"recon of plane {k}")
        h8, w8 = _full(gr).shape
        assert not gr[h8:].any() and not gr[:, w8:].any(), f"plane {k}: recon outside full blocks is not 0"
    outside = ~_inside(n, sets)
    assert outside.any()
    assert (r[outside] == SENTINEL).all(), "a recon write outside the plane rectangles"
    assert (l[outside] == SENTINEL).all(), "a level write outside the plane rectangles"


def _layout(gpu, name):
    if name == "odd":       # nothing aligned: two planes side by side, pitch and group gaps, a base offset
        w, h, groups = 29, 37, 3
        pitch, base = 2 * w + 3, 5
        s = gpu.plane_set(base, w, h, pitch, planes_per_group=2, num_groups=groups, plane_stride=w,
                          group_stride=h * pitch + 11)
    else:                   # everything a multiple of 8 elements: the 16-byte paths
        w, h, groups = 40, 24, 2
        s = gpu.plane_set(16, w, h, 96, planes_per_group=2, num_groups=groups, plane_stride=48, group_stride=24 * 96)
    return [s], s.base + groups * s.group_stride + 9   # and a tail behind the last group


@pytest.mark.parametrize("name", ["odd", "aligned"])
def test_layout_decoder(torch, gpu, name):
    sets, n = _layout(gpu, name)
    _check_decoder(torch, gpu, sets, n, 27, 61)


@pytest.mark.parametrize("name", ["odd", "aligned"])
def test_layout_encoder(torch, gpu, name):
    sets, n = _layout(gpu, name)
    _check_encoder(torch, gpu, sets, n, 29, 62)


def _eight_sets(gpu, degenerate=False):
    """NH_MAX_PLANE_SETS sets with 0, 1, 2, 5, 3, 1, 4, 2 block rows (the first is 7 high), 1..3 planes
    each in mixed splits.  ``degenerate`` (decoder only): the tallest set has no group, so max_bh comes
    from a set without planes, and the 40-wide set is 5 wide, so its rows have no block."""
    widths = [24, 44, 8, 16, 29, 40, 32, 8]
    heights = [7, 13, 16, 44, 29, 8, 37, 20]
    split = [(1, 2), (1, 1), (3, 1), (1, 2), (1, 1), (1, 3), (2, 1), (1, 1)]   # (planes_per_group, num_groups)
    if degenerate:
        split[3] = (1, 0)
        widths[5] = 5
    sets, base = [], 3
    for k, (w, h, (ppg, groups)) in enumerate(zip(widths, heights, split)):
        if k == 6:   # side by side
            pitch, ps = 2 * w + 1, w
            gs = h * pitch + 4
        else:        # stacked, with gaps behind rows, planes and groups
            pitch = w + k % 3
            ps = h * pitch + k
            gs = ppg * ps + 2 * k + 1
        sets.append(gpu.plane_set(base, w, h, pitch, planes_per_group=ppg, num_groups=groups, plane_stride=ps,
                                  group_stride=gs))
        base += max(1, groups) * gs + 5
    assert [s.height // 8 for s in sets] == [0, 1, 2, 5, 3, 1, 4, 2]
    return sets, base


@pytest.mark.parametrize("degenerate", [False, True], ids=["plain", "degenerate"])
def test_eight_sets_decoder(torch, gpu, degenerate):
    sets, n = _eight_sets(gpu, degenerate)
    _check_decoder(torch, gpu, sets, n, 26, 71 + degenerate)


@pytest.mark.parametrize("wide", [False, True], ids=["packed", "32bit"])
def test_eight_sets_encoder(torch, gpu, wide):
    sets, n = _eight_sets(gpu)
    _check_encoder(torch, gpu, sets, n, 33, 73, wide=wide)


# ------------------------------------------------------------------ c. int16 wrap in the decoder

def _wrap_levels(qp):
    """A DC-only level whose flat residual is >= 32700 and one whose residual is <= -32700 (QP 22:
    level 16382 gives +32764), from a seeded scan of DC levels in +-70000.  The residual wraps
    through int16 as the level grows, so each target is hit by about 1 level in 1000: the scan stops
    at the first of each and allows 20000 candidates."""
    rng = np.random.default_rng(700 + qp)
    blk = np.zeros((8, 8), np.int32)
    hi = lo = None
    for v in rng.integers(-70000, 70001, 20000):
        blk[0, 0] = v
        r = residual_block(blk, qp)
        if hi is None and r.min() >= 32700:
            hi = int(v)
        if lo is None and r.max() <= -32700:
            lo = int(v)
        if hi is not None and lo is not None:
            return hi, lo
    raise AssertionError(f"QP {qp}: no DC level with a residual beyond +-32700 among 20000")


@pytest.mark.parametrize("qp", [22, 30, 51])
def test_decoder_int16_wrap(torch, gpu, qp):
    """reconstruct_block adds prediction and residual in int16: 200 + 32764 wraps to -32572 and clips
    to 0, not to 255.  Each block of a 48 x 48 plane gets a DC level whose residual is >= 32700, one
    whose residual is <= -32700, or a small DC, plus one small AC level.  A decoder that adds in 64
    bits and clips without wrapping must differ from ``decode`` at 200 or more of the 2304 samples
    (checked on the CPU first); the GPU must equal ``decode``.  Low QPs cannot reach the wrap with
    these levels: a DC level's residual is level * 2^((QP - 16) / 6) (QP 22: twice the level), so at
    QP 9 and below +-70000 stays under 32700; hence QPs from the upper range."""
    h = w = 48
    hi, lo = _wrap_levels(qp)
    rng = np.random.default_rng(900 + qp)
    modes = rng.integers(0, 35, (h // 8, w // 8)).astype(np.uint8)
    lvl = np.zeros((h, w), np.int32)
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            lvl[by, bx] = (hi, lo, int(rng.integers(-3, 4)))[int(rng.integers(0, 3))]
            ac = int(rng.integers(1, 64))
            lvl[by + ac // 8, bx + ac % 8] = int(rng.choice([-2, -1, 1, 2]))
    want = decode(modes, lvl, qp)
    no_wrap = decode(modes, lvl, qp, reconstruct=lambda pred, res: np.clip(
        pred.astype(np.int64) + res.astype(np.int64), 0, 255).astype(np.int16))
    differ = int((no_wrap != want).sum())
    print(f"QP {qp}: levels {hi} / {lo}; a decoder without the int16 wrap differs at {differ} of {want.size} samples")
    assert differ >= 200
    got = _decode_gpu(torch, gpu, modes.ravel(), lvl.ravel(), [gpu.plane_set(0, w, h, w)], qp)
    _same(got, want, "recon")
