"""GPU parity of config 5 over its block pairings, its wide rule, its level bound,
its layouts and its per-set flag word: tc32_plane, tc32_planes (variants 0, 1, 2), tc32_planes_compact
(int16 / int8 levels) and tc32_levels_widen.  Fixtures: tests/tc32_matrix.py, checked on the CPU by
test_tc32_matrix_host.py.

Every output buffer starts as a sentinel; the comparison is bit-exact and against the pinned oracle
(oracle.tc32_plane on each plane's own 2-D view), never another GPU path.  A mismatch names the case,
the output, the first differing sample, its block, the block's (workgroup, wave, first / second block
of the wave) and whether the wide rule calls the block wide or narrow."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tc32_matrix as M  # noqa: E402

CASE_IDS = [c.name for c in M.CASES]
ALL_QPS = tuple(sorted(set(M.QPS + M.QPS_INT16)))
PAD = -4000           # source padding: a wide value no block may read


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


def _same(case, what, name, got, want, src, at=(0, 0)):
    msg = M.describe(case, name, got, want, src, at)
    if msg:
        pytest.fail(f"{what}: {msg}", pytrace=False)


def _sentinel(torch, dtype):
    return M.SENTINEL8 if dtype == torch.int8 else M.SENTINEL


def _full(torch, n, dtype, value=None):
    return torch.full((n,), _sentinel(torch, dtype) if value is None else value, dtype=dtype, device="cuda")


class Placed:
    """One plane set of a buffer: its case, layout, plane offsets and plane kinds."""

    def __init__(self, gpu, case, lay, ppg, groups, kinds):
        assert len(kinds) == ppg * groups
        self.case, self.lay, self.kinds = case, lay, kinds
        self.offs = M.plane_offsets(lay, ppg, groups)
        self.set = gpu.plane_set(lay.base, case.w, case.h, lay.pitch, ppg, groups, lay.plane_stride, lay.group_stride)

    def fill(self, buf):
        for off, kind in zip(self.offs, self.kinds):
            M.view(buf, self.case, self.lay, off)[:] = M.source(self.case, kind)


def _source(torch, placed, size):
    buf = np.full(size, PAD, np.int16)
    for p in placed:
        p.fill(buf)
    return torch.from_numpy(buf).cuda()


def _outside(placed, size):
    m = np.ones(size, bool)
    for p in placed:
        m &= np.concatenate([M.outside_full_mask(p.case, p.lay, p.offs), np.ones(size - p.lay.size, bool)])
    return m


def _check_int32(what, placed, qp, lvl, rec, fill=None):
    """Levels and recon of every plane equal the oracle's on the full blocks; every other element of the
    buffers keeps its sentinel (``fill``: what the buffers held)."""
    for p in placed:
        for k, (off, kind) in enumerate(zip(p.offs, p.kinds)):
            want = M.reference(p.case, kind, qp)
            for name, buf, ref in (("lvl", lvl, want[0]), ("rec", rec, want[1])):
                _same(p.case, f"{what}, QP {qp}, plane {k} ({kind})", name, M.full(p.case, M.view(buf, p.case, p.lay, off)),
                      M.full(p.case, ref), M.source(p.case, kind))
    out = _outside(placed, lvl.size)
    for name, buf in (("lvl", lvl), ("rec", rec)):
        keep = M.SENTINEL if fill is None else fill[name]
        assert (buf[out] == keep).all(), f"{what}, QP {qp}: {name} written outside the full blocks"


def _check_compact(what, placed, qp, cv, spill, lb):
    """Per full block: a block the rule calls wide has the marker at its compact origin and its int32 levels
    in the spill plane; every other block holds the oracle's levels (no marker: |level| <= 51)."""
    for p in placed:
        case = p.case
        for k, (off, kind) in enumerate(zip(p.offs, p.kinds)):
            src = M.source(case, kind)
            want = M.reference(case, kind, qp)[0]
            C, S = M.view(cv, case, p.lay, off), M.view(spill, case, p.lay, off)
            tag = f"{what}, QP {qp}, plane {k} ({kind})"
            for b, wide in enumerate(M.block_wide(case, src)):
                y0, x0 = M.block_origin(case, b)
                blk, ref = C[y0:y0 + 32, x0:x0 + 32], want[y0:y0 + 32, x0:x0 + 32]
                g, w, second = M.wave_of(b)
                where = f"{case.name}: {tag}: block {b} (workgroup {g}, wave {w}, its {'second' if second else 'first'} block)"
                if wide:
                    assert blk[0, 0] == M.MARK[lb], f"{where} is wide by the rule and has no marker"
                    _same(case, tag, "spill", S[y0:y0 + 32, x0:x0 + 32], ref, src, at=(y0, x0))
                else:
                    assert np.abs(ref).max() <= 51
                    assert not (blk == M.MARK[lb]).any(), f"{where} is narrow by the rule and holds a marker"
                    _same(case, tag, "compact lvl", blk, ref.astype(cv.dtype), src, at=(y0, x0))


def _run_int32(torch, gpu, what, placed, d, qp, variant, stream=None, rec_fill=None, sets=None):
    lvl, rec = _full(torch, d.numel(), torch.int32), _full(torch, d.numel(), torch.int16, rec_fill)
    got = gpu.tc32_planes(d, sets or [p.set for p in placed], qp, variant, lvl=lvl, rec=rec, stream=stream)
    assert got[0] is lvl and got[1] is rec
    if stream is not None:
        stream.synchronize()
    fill = None if rec_fill is None else {"lvl": M.SENTINEL, "rec": rec_fill}
    _check_int32(what, placed, qp, lvl.cpu().numpy(), rec.cpu().numpy(), fill)


def _run_compact(torch, gpu, what, placed, d, qp, dt, stream=None, rec_fill=None, sets=None):
    """tc32_planes_compact + tc32_levels_widen: recon and widened levels equal the oracle, the compact levels
    and the spill plane are as ``_check_compact`` says; nothing is written outside the full blocks."""
    n, sets = d.numel(), sets or [p.set for p in placed]
    lc, rc = _full(torch, n, dt), _full(torch, n, torch.int16, rec_fill)
    spill, wide = _full(torch, n, torch.int32), _full(torch, n, torch.int32)
    got = gpu.tc32_planes_compact(d, sets, qp, dt, lvl=lc, rec=rc, spill=spill, stream=stream)
    assert got[0] is lc and got[1] is rc and got[2] is spill
    assert gpu.tc32_levels_widen(lc, spill, sets, out=wide, stream=stream) is wide
    if stream is not None:
        stream.synchronize()
    cv, sv = lc.cpu().numpy(), spill.cpu().numpy()
    fill = None if rec_fill is None else {"lvl": M.SENTINEL, "rec": rec_fill}
    _check_int32(what + ", widened", placed, qp, wide.cpu().numpy(), rc.cpu().numpy(), fill)
    _check_compact(what, placed, qp, cv, sv, lc.element_size())
    out = _outside(placed, n)
    assert (cv[out] == _sentinel(torch, dt)).all(), f"{what}, QP {qp}: compact levels written outside the full blocks"
    assert (sv[out] == M.SENTINEL).all(), f"{what}, QP {qp}: spill written outside the full blocks"
    return cv


def _modes(torch):
    return {"int32": None, "int16": torch.int16, "int8": torch.int8}


def _run(torch, gpu, what, placed, d, qp, mode, **kw):
    dt = _modes(torch)[mode]
    if dt is None:
        return _run_int32(torch, gpu, f"{what}, variant 1", placed, d, qp, 1, **kw)
    return _run_compact(torch, gpu, f"{what}, {mode} levels", placed, d, qp, dt, **kw)


def _up16(n):
    return (n + 15) // 16 * 16


# ------------------------------------------------------------------ 1. geometry x planes x variants

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_geometry_planes_variants_vs_oracle(torch, gpu, case, variant):
    """Planes a .. f of every geometry case in one tc32_planes call per QP (six groups of one plane, the
    smallest 8-aligned pitch) and, where w % 8 == 0, each alone through tc32_plane."""
    lay = M.layout(case, 0, (case.w + 7) // 8 * 8, 1, len(M.KINDS))
    placed = [Placed(gpu, case, lay, 1, len(M.KINDS), M.KINDS)]
    d = _source(torch, placed, lay.size)
    for qp in ALL_QPS:
        _run_int32(torch, gpu, f"tc32_planes, variant {variant}", placed, d, qp, variant)
    if case.w % 8:
        return
    for kind in M.KINDS:
        src = M.source(case, kind)
        d1 = torch.from_numpy(np.array(src)).cuda()
        for qp in (M.QPS_INT16 if kind == "d" else M.QPS):
            lvl = torch.full(src.shape, M.SENTINEL, dtype=torch.int32, device="cuda")
            rec = torch.full(src.shape, M.SENTINEL, dtype=torch.int16, device="cuda")
            got = gpu.tc32_plane(d1, qp, variant, lvl=lvl, rec=rec)
            assert got[0] is lvl and got[1] is rec
            want = M.reference(case, kind, qp)
            outside = ~M.full_mask(case)
            for name, t, ref in (("lvl", lvl, want[0]), ("rec", rec, want[1])):
                a = t.cpu().numpy()
                _same(case, f"tc32_plane, variant {variant}, QP {qp}, plane {kind}", name, M.full(case, a), M.full(case, ref), src)
                assert (a[outside] == M.SENTINEL).all(), (case.name, kind, qp, name, "written outside the full blocks")


# ------------------------------------------------------------------ 2. pairing and wide rule

@pytest.mark.parametrize("mode", ["int32", "int16", "int8"])
@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_pairing_and_wide_rule_vs_oracle(torch, gpu, case, mode):
    """Plane c and every single-plant plane of the case, NAME and NAME!.  On the pairing case: every wave
    form (narrow / wide first block x narrow / wide / no second block).  On every case: blocks wide through
    their top row or left column alone -- in a one-column plane, in a one-row plane, as a wave's lone block --
    and plants that must leave a block narrow.  A near plant wrongly left narrow shows as a missing marker
    in the compact levels, a far one in the outputs; a block wrongly turned wide as a marker over the
    oracle's levels."""
    kinds = ("c",) + M.single_kinds(case)
    lay = M.layout(case, 16, _up16(case.w), 1, len(kinds))
    placed = [Placed(gpu, case, lay, 1, len(kinds), kinds)]
    d = _source(torch, placed, lay.size)
    for qp in (0, 22):
        _run(torch, gpu, "wide rule", placed, d, qp, mode)


# ------------------------------------------------------------------ 3. level bound

@pytest.mark.parametrize("mode", ["int32", "int16", "int8"])
@pytest.mark.parametrize("case", [M.BY_NAME["2x3"], M.PAIRING], ids=["2x3", "11x2"])
def test_level_bound_vs_oracle(torch, gpu, case, mode):
    """Plane f: levels +51 and -51 at QP 0, the bound of the int8 levels, next to the marker -128."""
    lay = M.layout(case, 0, _up16(case.w), 1, 1)
    placed = [Placed(gpu, case, lay, 1, 1, ("f",))]
    d = _source(torch, placed, lay.size)
    for qp in (0, 1, 4, 22):
        cv = _run(torch, gpu, "plane f", placed, d, qp, mode)
        if qp == 0 and mode != "int32":
            C = M.full(case, M.view(cv, case, lay, 0))
            assert C.max() == 51 and C.min() == -51, (case.name, mode, int(C.max()), int(C.min()))


# ------------------------------------------------------------------ 4. layouts

LAYOUT_KINDS = ("a", "c", "d", "e", "f", "right_edge!")


def _layout_case(gpu, case, aligned16):
    """Two groups of three planes with a gap behind every plane and every group, pitch > width, base > 0:
    everything 16-element aligned, or 8- but not 16-element aligned."""
    if aligned16:
        lay = M.layout(case, 32, _up16(case.w + 1), 3, 2, gap=16, group_gap=48)
        assert not (lay.base | lay.pitch | lay.plane_stride | lay.group_stride) & 15
    else:
        pitch = _up16(case.w + 1) + 8
        lay = M.layout(case, 8, pitch, 3, 2, gap=8 if (case.h * pitch) % 16 == 0 else 16, group_gap=24)
        assert not (lay.base | lay.pitch | lay.plane_stride | lay.group_stride) & 7
        assert lay.base & 15 and lay.pitch & 15 and lay.plane_stride & 15
    assert lay.pitch > case.w
    return [Placed(gpu, case, lay, 3, 2, LAYOUT_KINDS)], lay


@pytest.mark.parametrize("aligned16", [True, False], ids=["16-aligned", "8-aligned"])
@pytest.mark.parametrize("case", [M.BY_NAME["2x3"], M.BY_NAME["5x2"]], ids=["2x3", "5x2"])
def test_layouts_vs_oracle(torch, gpu, case, aligned16):
    """8-bit, mixed, int16 and single-plant planes in one launch (blockIdx.y), source padding a wide value."""
    placed, lay = _layout_case(gpu, case, aligned16)
    d = _source(torch, placed, lay.size)
    for qp in (0, 22):
        for variant in (0, 1, 2):
            _run_int32(torch, gpu, f"layout, variant {variant}", placed, d, qp, variant)
        _run(torch, gpu, "layout", placed, d, qp, "int16")
        if aligned16:
            _run(torch, gpu, "layout", placed, d, qp, "int8")
    if not aligned16:      # int8 levels need 16-element aligned rows, planes and groups
        n = d.numel()
        bufs = [_full(torch, n, torch.int8), _full(torch, n, torch.int16), _full(torch, n, torch.int32)]
        with pytest.raises(ValueError):
            gpu.tc32_planes_compact(d, [placed[0].set], 22, torch.int8, lvl=bufs[0], rec=bufs[1], spill=bufs[2])
        for t in bufs:
            assert bool((t == _sentinel(torch, t.dtype)).all()), "a refused call wrote"


@pytest.mark.parametrize("mode", ["int32", "int16", "int8"])
def test_layout_recon_prefilled_with_the_wide_mark(torch, gpu, mode):
    """Recon starts as -32768 everywhere, the value the narrow launch itself leaves at a wide block's origin
    for the fix-up: same outputs, and the padding is still -32768."""
    placed, lay = _layout_case(gpu, M.BY_NAME["5x2"], True)
    d = _source(torch, placed, lay.size)
    for qp in (0, 22):
        _run(torch, gpu, "recon pre-filled with -32768", placed, d, qp, mode, rec_fill=M.MARK_REC)


# ------------------------------------------------------------------ 5. sets and the flag word

def _eight_sets(gpu):
    """Eight sets of different sizes in one buffer: wide blocks in set 4 only (it also holds an 8-bit plane);
    set 1 has no full block, set 2 no group."""
    plan = [("1x1", 1, 1, ("a",)), (None, 1, 1, None), ("2x3", 1, 0, ()), ("2x3", 2, 1, ("b", "a")),
            ("5x2", 1, 3, ("c", "d", "a")), ("1x9", 1, 1, ("e",)), ("9x1", 2, 1, ("f", "b")), ("2x3", 1, 1, ("e",))]
    placed, sets, at = [], [], 16
    for name, ppg, groups, kinds in plan:
        if name is None:               # 24 x 40 samples: no full block
            sets.append(gpu.plane_set(at, 24, 40, 32))
            at += 40 * 32 + 16
            continue
        case = M.BY_NAME[name]
        lay = M.layout(case, at, _up16(case.w), ppg, groups, gap=16)
        if groups:
            placed.append(Placed(gpu, case, lay, ppg, groups, kinds))
            sets.append(placed[-1].set)
            at = lay.size + 16
        else:
            sets.append(gpu.plane_set(at, case.w, case.h, lay.pitch, ppg, 0, lay.plane_stride, lay.group_stride))
    assert len(sets) == 8 and len({(s.width, s.height, s.planes_per_group, s.num_groups) for s in sets}) >= 7
    wide = [any(any(M.block_wide(p.case, M.source(p.case, k))) for k in p.kinds) for p in placed]
    assert wide == [False, False, True, False, False, False]
    return placed, sets, at


@pytest.mark.parametrize("mode", ["int32", "int16", "int8"])
def test_eight_sets_one_call_vs_oracle(torch, gpu, mode):
    """Each set has its own launches and its own flag word: the fix-up of the wide set must run, those of
    the narrow sets before and after it must find nothing; the block-less and group-less sets write nothing."""
    placed, sets, size = _eight_sets(gpu)
    d = _source(torch, placed, size)
    for qp in (0, 22):
        _run(torch, gpu, "eight sets", placed, d, qp, mode, sets=sets)


@pytest.mark.parametrize("order", ["wide-then-narrow", "narrow-then-wide"])
@pytest.mark.parametrize("own_stream", [False, True], ids=["current-stream", "caller-stream"])
def test_narrow_and_wide_calls_back_to_back(torch, gpu, own_stream, order):
    """On one stream a call whose planes are all wide and a call whose planes are all 8-bit, one at once after
    the other, into fresh buffers.  Narrow after wide: the narrow call's fix-ups must not act on the wide
    call's flags.  Wide after narrow: the wide call's fix-ups must run -- a flag word or epoch left by the
    narrow call must not make them return early, which would leave the marks in the recon and the levels
    unwritten.  int32 and int16 levels; through the current stream and through a caller-made one."""
    case = M.BY_NAME["5x2"]
    pitch = _up16(case.w)
    wide = [Placed(gpu, case, M.layout(case, 0, pitch, 1, 3), 1, 3, ("d", "d", "d"))]
    narrow = [Placed(gpu, case, M.layout(case, 0, pitch, 1, 4), 1, 4, ("a", "b", "e", "f"))]
    assert all(M.block_wide(case, M.plane(case, "d"))) and not any(any(M.block_wide(case, M.plane(case, k))) for k in "abef")
    calls = [(_source(torch, wide, wide[0].lay.size), wide), (_source(torch, narrow, narrow[0].lay.size), narrow)]
    if order == "narrow-then-wide":
        calls.reverse()
    stream = torch.cuda.Stream() if own_stream else None
    for qp in (0, 22):
        for dt in (None, torch.int16):
            outs = []
            for d, placed in calls:
                n = d.numel()
                outs.append([_full(torch, n, dt or torch.int32), _full(torch, n, torch.int16), _full(torch, n, torch.int32),
                             _full(torch, n, torch.int32)])
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())      # the uploads and the fills above
            for (d, placed), (lvl, rec, spill, out) in zip(calls, outs):   # back to back
                sets = [p.set for p in placed]
                if dt is None:
                    gpu.tc32_planes(d, sets, qp, 1, lvl=lvl, rec=rec, stream=stream)
                else:
                    gpu.tc32_planes_compact(d, sets, qp, dt, lvl=lvl, rec=rec, spill=spill, stream=stream)
            for (d, placed), (lvl, rec, spill, out) in zip(calls, outs):
                if dt is not None:
                    gpu.tc32_levels_widen(lvl, spill, [p.set for p in placed], out=out, stream=stream)
            (torch.cuda.current_stream() if stream is None else stream).synchronize()
            for (d, placed), (lvl, rec, spill, out) in zip(calls, outs):
                what = f"{order}: {'all-wide' if placed is wide else 'all-8-bit'} call, {'int32' if dt is None else 'int16'} levels"
                _check_int32(what, placed, qp, (lvl if dt is None else out).cpu().numpy(), rec.cpu().numpy())
                if dt is not None:
                    _check_compact(what, placed, qp, lvl.cpu().numpy(), spill.cpu().numpy(), 2)


# ------------------------------------------------------------------ 6. refusals

def test_refusals_write_nothing(torch, gpu):
    """Each refused call raises before any write."""
    case = M.BY_NAME["2x3"]
    w, h, pitch = case.w, case.h, _up16(case.w)
    ok = Placed(gpu, case, M.layout(case, 16, pitch, 2, 2, gap=16), 2, 2, ("a", "c", "d", "f"))
    n = ok.lay.size
    d = _source(torch, [ok], n)
    bufs = {dt: _full(torch, n, dt) for dt in (torch.int32, torch.int16, torch.int8)}
    rec, spill, out = _full(torch, n, torch.int16), _full(torch, n, torch.int32), _full(torch, n, torch.int32)
    small32, small16 = _full(torch, n // 2, torch.int32), _full(torch, n // 2, torch.int16)
    ps = gpu.plane_set

    def refused(exc, fn, *a, **kw):
        with pytest.raises(exc):
            fn(*a, **kw)
        for t in list(bufs.values()) + [rec, spill, out, small32, small16]:
            assert bool((t == _sentinel(torch, t.dtype)).all()), "a refused call wrote"

    lvl = bufs[torch.int32]
    refused(ValueError, gpu.tc32_planes, d, [ok.set] * 9, 22, 1, lvl=lvl, rec=rec)                       # nsets = 9
    refused(ValueError, gpu.tc32_planes_compact, d, [ok.set] * 9, 22, torch.int16, lvl=bufs[torch.int16], rec=rec, spill=spill)
    refused(ValueError, gpu.tc32_levels_widen, bufs[torch.int16], spill, [ok.set] * 9, out=out)
    refused(ValueError, gpu.tc32_planes, d, [ok.set], 22, 3, lvl=lvl, rec=rec)                           # variant 3
    d2 = torch.from_numpy(np.array(M.plane(M.BY_NAME["1x9"], "a"))).cuda()
    l2 = torch.full(d2.shape, M.SENTINEL, dtype=torch.int32, device="cuda")
    r2 = torch.full(d2.shape, M.SENTINEL, dtype=torch.int16, device="cuda")
    refused(ValueError, gpu.tc32_plane, d2, 22, 3, lvl=l2, rec=r2)
    assert bool((l2 == M.SENTINEL).all()) and bool((r2 == M.SENTINEL).all())
    bad = {
        "pitch < width": ps(16, w, h, w - 12),
        "pitch not 8-aligned": ps(16, w, h, pitch + 4),
        "base not 8-aligned": ps(20, w, h, pitch),
        "plane stride not 8-aligned": ps(16, w, h, pitch, 2, 1, h * pitch + 4, 0),
        "group stride not 8-aligned": ps(16, w, h, pitch, 1, 2, 0, h * pitch + 4),
    }
    for why, s in bad.items():
        for variant in (0, 1, 2):
            refused(ValueError, gpu.tc32_planes, d, [ok.set, s], 22, variant, lvl=lvl, rec=rec)          # (after a good set)
        for dt in (torch.int16, torch.int8):
            refused(ValueError, gpu.tc32_planes_compact, d, [ok.set, s], 22, dt, lvl=bufs[dt], rec=rec, spill=spill)
    # compact levels of another dtype
    refused(TypeError, gpu.tc32_planes_compact, d, [ok.set], 22, torch.int32, lvl=lvl, rec=rec, spill=spill)
    refused(TypeError, gpu.tc32_planes_compact, d, [ok.set], 22, lvl=lvl, rec=rec, spill=spill)
    refused(TypeError, gpu.tc32_planes_compact, d, [ok.set], 22, torch.int16, lvl=bufs[torch.int8], rec=rec, spill=spill)
    refused(TypeError, gpu.tc32_levels_widen, lvl, spill, [ok.set], out=out)
    # buffers smaller than the source
    refused(ValueError, gpu.tc32_planes, d, [ok.set], 22, 1, lvl=small32, rec=rec)
    refused(ValueError, gpu.tc32_planes, d, [ok.set], 22, 1, lvl=lvl, rec=small16)
    refused(ValueError, gpu.tc32_planes_compact, d, [ok.set], 22, torch.int16, lvl=small16, rec=rec, spill=spill)
    refused(ValueError, gpu.tc32_planes_compact, d, [ok.set], 22, torch.int16, lvl=bufs[torch.int16], rec=rec, spill=small32)
    refused(ValueError, gpu.tc32_levels_widen, bufs[torch.int16], spill, [ok.set], out=small32)
    # a set that reaches outside the source
    refused(ValueError, gpu.tc32_planes, d, [ps(16, w, h, pitch, 2, 3, ok.lay.plane_stride, ok.lay.group_stride)], 22, 1,
            lvl=lvl, rec=rec)
    # ... and the good set alone is accepted
    _run_int32(torch, gpu, "the accepted set", [ok], d, 22, 1)
