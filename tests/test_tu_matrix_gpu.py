"""GPU parity of config 4 at EVERY (ctb, is_luma) its entry points accept:
open loop, plane sets, the per-size fallback and the closed loop at ctb 4 / 8 / 16 / 32 as luma and as
chroma; compact levels and the decoder family at the two pairs the other tests leave out, (32, chroma)
and (16, luma).  Fixtures: tests/tu_matrix.py, checked on the CPU by test_tu_matrix_host.py.

Every output buffer starts as a sentinel; the comparison is bit-exact and against the pinned oracle
(oracle.tu_pipeline_plane / tu_pipeline_plane_closed, tu_decode_ref.py), never another GPU path.  A
mismatch names the case, the output, the first differing sample and the TU that holds it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tu_decode_ref as R  # noqa: E402
import tu_matrix as M  # noqa: E402

CASE_IDS = [c.name for c in M.CASES]
MATRIX = [c for c in M.CASES if not c.name.endswith("-tall")]           # one case per (ctb, is_luma)
MATRIX_IDS = [c.name for c in MATRIX]
LEFT_OUT = [M.BY_NAME["ctb32-chroma"], M.BY_NAME["ctb16-luma"]]          # of the ctb 16 / 32 entry points' tests
LEFT_OUT_IDS = [c.name for c in LEFT_OUT]
MARK = -32768                                                            # compact levels: a wide strip's origin


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


def _same(case, what, name, got, want, tu, at=(0, 0)):
    msg = M.describe(case, name, got, want, tu, at)
    if msg:
        pytest.fail(f"{what}: {msg}", pytrace=False)


def _same3(case, what, got, want):
    """(levels, recon, TU map) against the oracle's; no marker bit survives in the map."""
    for name, g, w in zip(("tu", "lvl", "rec"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
        _same(case, what, name, g, w, want[2])
    assert not (got[2] & 0x80).any(), what


def _outputs(torch, shape_lr, shape_tu, lvl_dtype=None):
    lvl = torch.full(shape_lr, M.SENTINEL, dtype=lvl_dtype or torch.int32, device="cuda")
    rec = torch.full(shape_lr, M.SENTINEL, dtype=torch.int16, device="cuda")
    tu = torch.full(shape_tu, M.SENTINEL_TU, dtype=torch.uint8, device="cuda")
    return lvl, rec, tu


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the fixtures are read-only)


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


# ------------------------------------------------------------------ 1. open loop, one plane

def _open_runs(case):
    return [(k, qp) for k in M.KINDS_8BIT + ("c",) for qp in M.QPS] + [("d", M.QP_INT16)]


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_open_loop_vs_oracle_and_bands(torch, gpu, case):
    """Planes a .. e whole, then as CTU-row bands of 2 rows into shared outputs (the strips of a band are
    numbered from its first row: other groups, other trailing batches)."""
    h, w, pid = case.h, case.w, M.plane_id(case)
    rows = M.geometry(case).rows
    for kind, qp in _open_runs(case):
        what = f"open loop, plane {kind}, QP {qp}"
        d = _dev(torch, M.plane(case, kind))
        want = M.reference(case, kind, qp)
        out = _outputs(torch, (h, w), (h // 4, w // 4))
        got = gpu.tu_pipeline_plane(d, case.ctb, pid, case.seed, qp, case.luma, lvl=out[0], rec=out[1], tu=out[2])
        _same3(case, what, _np(*got), want)
        out = _outputs(torch, (h, w), (h // 4, w // 4))
        for r0 in range(0, rows, 2):
            gpu.tu_pipeline_plane(d, case.ctb, pid, case.seed, qp, case.luma, r0, r0 + 2, lvl=out[0], rec=out[1], tu=out[2])
        _same3(case, what + ", bands of 2 CTU rows", _np(*out), want)


# ------------------------------------------------------------------ 2. plane sets, padded layout

def _set_outputs_same(case, what, lay, offs, kinds, pids, qp, got, closed=False):
    """Every plane of the layout equals its own oracle run; everything outside the planes is untouched."""
    lvl, rec, tu = got
    for k, (off, kind, pid) in enumerate(zip(offs, kinds, pids)):
        want = M.reference(case, kind, qp, closed, pid=pid)
        one = (M.view(lvl, case, lay, off), M.view(rec, case, lay, off), tu[k])
        _same3(case, f"{what}, plane {k} ({kind}, plane id {pid})", one, want)
    out = M.outside_mask(case, lay, offs)
    assert (lvl[out] == M.SENTINEL).all() and (rec[out] == M.SENTINEL).all(), f"{case.name}: {what}: padding written"


@pytest.mark.parametrize("case", MATRIX, ids=MATRIX_IDS)
def test_plane_sets_padded_vs_oracle(torch, gpu, case):
    """One call over 2 groups of 2 planes (plane ids pid, pid + 1) with pitch = w + 4: group 0 is 8-bit, the
    planes of group 1 hold ONE wide sample each -- in the last column of a strip, so the strip to its right
    is wide through its left column alone, and in the last row of a strip, so the strip below is wide
    through its top row alone (in another group than the planted strip: below at every CTB, to the right at
    CTB 32); the value is tu_matrix.FAR, which the packed chain of a group wrongly left narrow cannot
    predict from.  The pitch padding of an 8-bit plane holds a wide value no strip may read."""
    pid, qp = M.plane_id(case), case.qp
    kinds, pids = ("a", "b", "right_edge!", "bottom_edge!"), (pid, pid + 1, pid, pid + 1)
    lay = M.layout(case, 4, case.w + 4, 2, 2, gap=8)
    offs = M.plane_offsets(lay, 2, 2)
    buf = M.fill(case, lay, [M.source(case, k) for k in kinds], offs, pad_value=77)
    y = min(case.ctb, case.h - 1)
    buf[offs[0] + y * lay.pitch + case.w] = 4000          # right of plane a's row y: left of no strip
    buf[offs[1] - 1] = -4000                              # in front of plane b: above no strip
    ps = gpu.plane_set(lay.base, case.w, case.h, lay.pitch, 2, 2, lay.plane_stride, lay.group_stride)
    lvl, rec, tu = _outputs(torch, (lay.size,), (4, case.h // 4, case.w // 4))
    got = gpu.tu_pipeline_planes(torch.from_numpy(buf).cuda(), ps, case.ctb, pid, case.seed, qp, case.luma,
                                 lvl=lvl, rec=rec, tu=tu)
    assert got[0] is lvl and got[1] is rec and got[2] is tu
    _set_outputs_same(case, "plane set, pitch w + 4", lay, offs, kinds, pids, qp, _np(lvl, rec, tu))


# ------------------------------------------------------------------ 3. the per-size fallback

@pytest.mark.parametrize("how", ["pitch+2", "base+2"])
@pytest.mark.parametrize("case", MATRIX, ids=MATRIX_IDS)
def test_layout_fallback_vs_oracle(torch, gpu, case, how):
    """Layouts the CTU-granular launch refuses (a pitch that is no multiple of 4, a base 2 elements off): the
    per-size launches code the set, every size up to ctb, 8-bit, mixed and int16 planes."""
    pid = M.plane_id(case)
    kinds = ("a", "c", "d")
    lay = M.layout(case, *((0, case.w + 2) if how == "pitch+2" else (2, case.w)), 1, 3, gap=6)
    assert lay.pitch % 4 or lay.base % 4
    offs = M.plane_offsets(lay, 1, 3)
    buf = M.fill(case, lay, [M.plane(case, k) for k in kinds], offs, pad_value=77)
    ps = gpu.plane_set(lay.base, case.w, case.h, lay.pitch, 1, 3, lay.plane_stride, lay.group_stride)
    d = torch.from_numpy(buf).cuda()
    for qp in (case.qp, M.QP_INT16):
        lvl, rec, tu = _outputs(torch, (lay.size,), (3, case.h // 4, case.w // 4))
        gpu.tu_pipeline_planes(d, ps, case.ctb, pid, case.seed, qp, case.luma, lvl=lvl, rec=rec, tu=tu)
        _set_outputs_same(case, f"fallback ({how}), QP {qp}", lay, offs, kinds, (pid,) * 3, qp, _np(lvl, rec, tu))


# ------------------------------------------------------------------ 4. compact levels

@pytest.mark.parametrize("qp", M.QPS)
@pytest.mark.parametrize("case", LEFT_OUT, ids=LEFT_OUT_IDS)
def test_compact_levels_vs_oracle(torch, gpu, case, qp):
    """int16 levels over an 8-bit plane, an int16 plane, the mixed plane c and the planes with one wide
    sample at a strip's edge (the values next to 0..255: -1 left of a strip, 256 above one) in a padded
    layout: the widened levels, recon and TU maps are the oracle's; every strip of a narrow group (the rule restated in
    tu_matrix.group_wide) holds the oracle's levels, |level| <= 408, every strip of a wide group the marker
    at its origin; a wide value in plane a's pitch padding marks nothing; a CTU-row band widens alone."""
    pid, ctb = M.plane_id(case), case.ctb
    g = M.geometry(case)
    kinds = ("a", "d", "c", "right_edge", "bottom_edge")
    n = len(kinds)
    assert M.plants(case)["right_edge"][2] == -1 and M.plants(case)["bottom_edge"][2] == 256
    lay = M.layout(case, 8, (case.w + 15) // 8 * 8, 1, n, gap=16)
    assert lay.pitch > case.w and not (lay.pitch | lay.base | lay.plane_stride | lay.group_stride) & 7
    offs = M.plane_offsets(lay, 1, n)
    buf = M.fill(case, lay, [M.source(case, k) for k in kinds], offs, pad_value=77)
    buf[offs[0] + (ctb + 1) * lay.pitch + case.w] = -4000         # right of plane a, beside the last strip of a row
    ps = gpu.plane_set(lay.base, case.w, case.h, lay.pitch, 1, n, lay.plane_stride, lay.group_stride)
    d = torch.from_numpy(buf).cuda()
    lc, rc, tu = _outputs(torch, (lay.size,), (n, case.h // 4, case.w // 4), lvl_dtype=torch.int16)
    spill = torch.full((lay.size,), M.SENTINEL, dtype=torch.int32, device="cuda")
    gpu.tu_pipeline_planes_compact(d, ps, ctb, pid, case.seed, qp, case.luma, lvl=lc, rec=rc, tu=tu, spill=spill)
    wide = torch.full((lay.size,), M.SENTINEL, dtype=torch.int32, device="cuda")
    assert gpu.tu_levels_widen(lc, spill, ps, ctb, out=wide) is wide
    band = torch.full((lay.size,), M.SENTINEL, dtype=torch.int32, device="cuda")
    gpu.tu_levels_widen(lc, spill, ps, ctb, 1, 3, out=band)
    cv, rv, tv, wv, bv = _np(lc, rc, tu, wide, band)
    what = f"compact levels, QP {qp}"
    _set_outputs_same(case, what + ", widened", lay, offs, kinds, (pid,) * n, qp, (wv, rv, tv))
    out = M.outside_mask(case, lay, offs)
    assert (cv[out] == M.SENTINEL).all() and (bv[out] == M.SENTINEL).all(), what + ": padding written"
    for k, (off, kind) in enumerate(zip(offs, kinds)):
        want = M.reference(case, kind, qp)[0]
        C, B = M.view(cv, case, lay, off), M.view(bv, case, lay, off)
        gw = M.group_wide(case, M.source(case, kind))
        assert {"a": not any(gw), "d": all(gw)}.get(kind, any(gw) and not all(gw))
        for s in range(g.strips):
            y0, x0 = M.strip_origin(case, s)
            blk, ref = C[y0:y0 + ctb, x0:x0 + g.sw], want[y0:y0 + ctb, x0:x0 + g.sw]
            if gw[s // 4]:
                assert blk[0, 0] == MARK, f"{case.name}: {what}: plane {kind}: strip {s} of a wide group has no marker"
            else:
                assert np.abs(ref).max() <= 408
                _same(case, f"{what}: plane {kind}: int16 levels of narrow strip {s}", "lvl", blk, ref.astype(np.int16),
                      M.tu_map(case), at=(y0, x0))
        _same(case, f"{what}: plane {kind}: band of CTU rows 1, 2", "lvl", B[ctb:3 * ctb], want[ctb:3 * ctb],
              M.tu_map(case), at=(ctb, 0))
        assert (B[:ctb] == M.SENTINEL).all() and (B[3 * ctb:] == M.SENTINEL).all(), what + ": band wrote other rows"


# ------------------------------------------------------------------ 5. closed loop

# (kinds, planes per group, groups): two groups of 8-bit planes take the packed plane-pair form, one
# group of two 8-bit planes (plane ids pid, pid + 1) the packed one-plane form, a set with a wide
# sample the 32-bit form
CLOSED_SETS = ((("a", "b"), 1, 2), (("b", "a"), 2, 1), (("c", "a"), 1, 2), (("a", "c"), 2, 1))


def _closed(torch, gpu, case, kinds, ppg, groups, qp):
    pid = M.plane_id(case)
    lay = M.layout(case, 0, case.w, ppg, groups)
    offs = M.plane_offsets(lay, ppg, groups)
    buf = M.fill(case, lay, [M.plane(case, k) for k in kinds], offs)
    ps = gpu.plane_set(0, case.w, case.h, case.w, ppg, groups, lay.plane_stride, lay.group_stride)
    d = torch.from_numpy(buf).cuda()
    lvl, rec, tu = _outputs(torch, (lay.size,), (len(kinds), case.h // 4, case.w // 4))
    got = gpu.tu_pipeline_closed(d, ps, case.ctb, pid, case.seed, qp, case.luma, lvl=lvl, rec=rec, tu=tu)
    assert got[0] is lvl and got[1] is rec and got[2] is tu
    pids = tuple(pid + (k % ppg) for k in range(len(kinds)))
    return d, ps, lay, offs, pids, (lvl, rec, tu)


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_closed_loop_vs_oracle(torch, gpu, case):
    for kinds, ppg, groups in CLOSED_SETS:
        for qp in ((0, case.qp) if kinds == ("a", "b") else (case.qp,)):
            _, _, lay, offs, pids, out = _closed(torch, gpu, case, kinds, ppg, groups, qp)
            _set_outputs_same(case, f"closed loop, planes {kinds}, {groups} group(s) of {ppg}, QP {qp}", lay, offs, kinds,
                              pids, qp, _np(*out), closed=True)


@pytest.mark.parametrize("case", M.CLOSED_ALIGNED, ids=[c.name for c in M.CLOSED_ALIGNED])
def test_closed_loop_pairs_aligned_width_vs_oracle(torch, gpu, case):
    """Five groups of one 8-bit plane, w % 8 == 0: the plane-pair form with its LDS source tile (CTB 8, 16),
    planes in twos or fours per wave and a short last bunch; the buffer ends with the last plane."""
    kinds = ("a", "b", "e", "b", "a")
    _, _, lay, offs, pids, out = _closed(torch, gpu, case, kinds, 1, 5, case.qp)
    assert lay.size == 5 * case.h * case.w
    _set_outputs_same(case, "closed loop, 5 groups, w % 8 == 0", lay, offs, kinds, pids, case.qp, _np(*out), closed=True)


# ------------------------------------------------------------------ 6. the decoder family

def _stage_r(torch, gpu, case, lvl2d, tu, qp, base, pitch):
    """``gpu.dequant_inv_tu`` on one plane at (base, pitch); nothing outside the plane is written."""
    lay = M.Layout(base, pitch, case.h * pitch, case.h * pitch, base + case.h * pitch + 5)
    ps = gpu.plane_set(base, case.w, case.h, pitch)
    buf = np.zeros(lay.size, lvl2d.dtype)
    M.view(buf, case, lay, base)[:] = lvl2d
    out = torch.full(buf.shape, M.SENTINEL, dtype=torch.int16, device="cuda")
    assert gpu.dequant_inv_tu(torch.from_numpy(buf).cuda(), torch.from_numpy(tu).cuda(), ps, case.ctb, case.luma, qp,
                              out=out) is out
    out = out.cpu().numpy()
    assert (out[M.outside_mask(case, lay, [base])] == M.SENTINEL).all()
    return M.view(out, case, lay, base).copy()


@pytest.mark.parametrize("case", LEFT_OUT, ids=LEFT_OUT_IDS)
def test_decoder_family_vs_cpu(torch, gpu, case):
    """From the closed-loop encoder's outputs on planes a, b and c: the pred-mode map, stage R on int32 and
    int16 levels in an aligned and in a (base 3, pitch w + 5) layout, and the decoder's reconstruction."""
    ctb, qp, h, w = case.ctb, case.qp, case.h, case.w
    choices = set()
    for kind in ("a", "b", "c"):
        what = f"decoder family, plane {kind}"
        d, ps, lay, offs, pids, out = _closed(torch, gpu, case, (kind,), 1, 1, qp)
        src = M.plane(case, kind)
        want = M.reference(case, kind, qp, closed=True)
        lvl, rec, tu = (a.reshape(s) for a, s in zip(_np(*out), ((h, w), (h, w), (h // 4, w // 4))))
        _same3(case, what + ", encoder", (lvl, rec, tu), want)
        assert R.valid(tu, ctb)
        pm = torch.full(out[2].shape, 7, dtype=torch.uint8, device="cuda")
        assert gpu.tu_pred_map_closed(d, out[1], out[2], ps, ctb, pm=pm) is pm
        want_pm = R.pred_map(src, rec, tu, ctb)
        _same(case, what, "tu", pm.cpu().numpy()[0], want_pm, tu)       # (a per-unit map: located like the TU map)
        choices |= set(np.unique(want_pm).tolist())
        want_res = R.residual(lvl, tu, ctb, qp, case.luma)
        l16 = lvl.astype(np.int16)
        assert np.array_equal(l16, lvl)
        for levels in (lvl, l16):
            for base, pitch in ((0, w), (3, w + 5)):
                _same(case, f"{what}, stage R on {levels.dtype} levels, base {base}, pitch {pitch}", "rec",
                      _stage_r(torch, gpu, case, levels, tu, qp, base, pitch), want_res, tu)
        dec = torch.full((h * w,), M.SENTINEL, dtype=torch.int16, device="cuda")
        assert gpu.tu_decode_closed(out[2], pm, out[0], ps, ctb, qp, case.luma, rec=dec) is dec
        dec = dec.cpu().numpy().reshape(h, w)
        _same(case, what + ", decoder", "rec", dec, R.decode(tu, want_pm, lvl, ctb, qp, case.luma), tu)
        _same(case, what + ", decoder against the encoder's recon", "rec", dec, rec, tu)
    assert choices == {0, 1}
