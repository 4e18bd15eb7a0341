"""Test helper: config 4 at EVERY (ctb, is_luma) its entry points accept,
ctb 4 / 8 / 16 / 32 as luma and as chroma.  CPU only, built on the pinned oracle and tu_decode_ref.py;
test_tu_matrix_host.py checks the conditions below with the oracle alone, test_tu_matrix_gpu.py runs
the cases on the GPU.

The open-loop kernel (nh_ctu.hip) works in STRIPS of 1024 / ctb columns x ctb rows, numbered in raster
order over the call's CTU rows, and GROUPS of 4 consecutive strips; a group pools its TU origins per
size and codes them in batches of 64 / N TUs (32 x 32 chroma TUs: 2 per batch).  Each case is the
smallest plane with two strips across, a partial last strip column, a partial last CTU row (not at
ctb 4: h % 4 == 0), a strip count that is no multiple of 4 and at least two groups, on which every TU
size up to ctb occurs, every size leaves some group a partial trailing batch and 4 x 4 TUs fill more
than one batch of some group.

Planes of a case (all int16):
  a  8-bit gradient + noise;
  b  samples 0 / 255 only;
  c  plane a with the wide samples of ``plants`` (outside 0..255);
  d  full-range int16 noise;
  e  8-bit noise with a patch of 128 over whole CTUs at the top-left corner: DC and planar tie there.
A group is WIDE (32-bit chain) when a sample of one of its strips, of the row above a strip or of the
column left of a strip is outside 0..255 (``strip_reasons``, restated here from that rule).  Plane c
plants one such sample in a strip's interior, in the last column of a strip (the strip to its right
turns wide through its left column alone), in the last row of a strip (the strip below through its top
row alone) and at the plane's last sample; ``plane_c_single`` holds one of them alone."""
import collections
import functools

import numpy as np

import tu_decode_ref as R
from oracle import oracle as O

SENTINEL = -12345
SENTINEL_TU = 0x5A

# patch: plane e's constant patch in CTUs (columns, rows)
Case = collections.namedtuple("Case", "name ctb luma w h seed qp patch")


def _case(ctb, luma, w, h, seed, qp, patch, tag=""):
    return Case(f"ctb{ctb}-{'luma' if luma else 'chroma'}{tag}", ctb, luma, w, h, seed, qp, patch)


# seeds, sizes and patches found on the CPU (test_tu_matrix_host.py asserts every condition)
CASES = (
    _case(4, True, 268, 44, 77, 22, (8, 1)),
    _case(4, False, 268, 44, 77, 22, (8, 1)),
    _case(8, True, 140, 52, 77, 22, (4, 2)),
    _case(8, False, 140, 52, 77, 22, (4, 2)),
    _case(16, True, 100, 68, 77, 22, (3, 2)),
    _case(16, False, 100, 68, 77, 22, (3, 2)),
    _case(32, True, 72, 136, 77, 22, (2, 2)),
    _case(32, False, 72, 136, 77, 22, (2, 2)),
    # 66 strips, 17 groups: the wide pass's second workgroup (16 groups each) has work
    _case(4, True, 268, 132, 77, 22, (8, 1), "-tall"),
)
BY_NAME = {c.name: c for c in CASES}
# Closed loop only: widths that are multiples of 8.  With two or more groups of such 8-bit planes the
# plane-pair kernel loads each CTU's source through an LDS tile in 16-byte pieces (CTB 8, 16, 32; at CTB 4
# a CTU origin is no multiple of 8 samples and the chains load from global memory); the cases above have
# w % 8 == 4 at CTB 4, 8 and 16 and never take that form.
CLOSED_ALIGNED = (
    _case(4, True, 72, 44, 77, 22, (1, 1), "-w72"),
    _case(8, False, 72, 44, 77, 22, (1, 1), "-w72"),
    _case(16, True, 72, 40, 77, 22, (1, 1), "-w72"),
)
QPS = (0, 22, 51)       # on the 8-bit planes
QP_INT16 = 3            # on plane d
KINDS_8BIT = ("a", "b", "e")
KINDS_WIDE = ("c", "d")


def plane_id(case):
    return 0 if case.luma else 1


Geometry = collections.namedtuple("Geometry", "sw strips_x rows strips groups")


def geometry(case):
    sw = 1024 // case.ctb
    sx, rows = -(-case.w // sw), -(-case.h // case.ctb)
    return Geometry(sw, sx, rows, sx * rows, -(-sx * rows // 4))


def strip_origin(case, s):
    g = geometry(case)
    return (s // g.strips_x) * case.ctb, (s % g.strips_x) * g.sw     # (y, x)


def strip_at(case, y, x):
    g = geometry(case)
    return (y // case.ctb) * g.strips_x + x // g.sw


# ------------------------------------------------------------------ planes

def _ro(a):
    a.setflags(write=False)
    return a


def _rng(case, salt):
    return np.random.default_rng([case.seed, case.ctb, int(case.luma), case.h, salt])


@functools.lru_cache(maxsize=None)
def plane(case, kind):
    """Read-only plane ``kind`` (a .. e) of the case."""
    h, w = case.h, case.w
    if kind == "a":
        yy, xx = np.mgrid[0:h, 0:w]
        return _ro(np.clip(70 + (xx + 2 * yy) % 140 + _rng(case, 1).integers(-20, 21, (h, w)), 0, 255).astype(np.int16))
    if kind == "b":
        return _ro((_rng(case, 2).integers(0, 2, (h, w)) * 255).astype(np.int16))
    if kind == "c":
        p = plane(case, "a").copy()
        for y, x, v in plants(case).values():
            p[y, x] = v
        return _ro(p)
    if kind == "d":
        return _ro(_rng(case, 4).integers(-32768, 32768, (h, w)).astype(np.int16))
    assert kind == "e"
    p = _rng(case, 5).integers(0, 256, (h, w)).astype(np.int16)
    p[:case.patch[1] * case.ctb, :case.patch[0] * case.ctb] = 128
    return _ro(p)


# A 9-bit value or -1 next to an 8-bit strip stays inside what the packed 16-bit chain computes exactly (its
# numerators stay below 2^15), so a group wrongly left narrow would still give the right outputs and only its
# missing compact-levels marker would show.  FAR is far enough outside that the packed chain cannot: a
# prediction from it differs from the oracle's whatever mode wins.
FAR = -20000


@functools.lru_cache(maxsize=None)
def plane_c_single(case, name, value=None):
    """Plane a with the one wide sample ``name`` of ``plants`` (``value``: instead of the table's)."""
    p = plane(case, "a").copy()
    y, x, v = plants(case)[name]
    p[y, x] = v if value is None else value
    return _ro(p)


# ------------------------------------------------------------------ the wide rule

def _pick(cands, prefer):
    """The highest strip of ``cands`` that ``prefer`` holds for, else the highest of all: the plants
    cluster at the plane's end and group 0 stays narrow."""
    good = [s for s in cands if prefer(s)]
    return max(good or cands)


@functools.lru_cache(maxsize=None)
def plant_strips(case):
    """(strip with the last-column plant, strip with the last-row plant): where the case allows it, the
    strip that turns wide through its halo lies in another group than the planted strip."""
    g = geometry(case)
    right = _pick([s for s in range(g.strips) if s % g.strips_x < g.strips_x - 1], lambda s: s // 4 != (s + 1) // 4)
    # (the last row of the strip must be a row of the plane: not the partial last CTU row)
    below = _pick([s for s in range(g.strips - g.strips_x)], lambda s: s // 4 != (s + g.strips_x) // 4)
    return right, below


@functools.lru_cache(maxsize=None)
def plants(case):
    """name -> (y, x, value) of plane c's wide samples: 9-bit positive and negative values."""
    g = geometry(case)
    right, below = plant_strips(case)
    ry, rx = strip_origin(case, right)
    by, bx = strip_origin(case, below)
    out = {
        # interior of the strip that also holds the last-column plant: not its first / last row or column
        "interior": (ry + min(case.ctb, case.h - ry) // 2, rx + g.sw // 2, 300),
        "right_edge": (ry + 1, rx + g.sw - 1, -1),
        "bottom_edge": (by + case.ctb - 1, bx + 5, 256),
        "last": (case.h - 1, case.w - 1, -300),
    }
    assert len({(y, x) for y, x, _ in out.values()}) == 4
    return out


def _wide(a):
    a = np.asarray(a)
    return bool(a.size) and bool(((a < 0) | (a > 255)).any())


def strip_reasons(case, src):
    """Per strip the set of reasons it is wide: 'own' (a sample of the strip), 'top' (the row above it,
    over its own columns), 'left' (the column left of it, over its own rows); 128 outside the plane."""
    g = geometry(case)
    out = []
    for s in range(g.strips):
        y0, x0 = strip_origin(case, s)
        y1, x1 = min(y0 + case.ctb, case.h), min(x0 + g.sw, case.w)
        why = set()
        if _wide(src[y0:y1, x0:x1]):
            why.add("own")
        if y0 > 0 and _wide(src[y0 - 1, x0:x1]):
            why.add("top")
        if x0 > 0 and _wide(src[y0:y1, x0 - 1]):
            why.add("left")
        out.append(why)
    return out


def group_wide(case, src):
    """Per group of 4 strips: coded by the 32-bit chain."""
    why = strip_reasons(case, src)
    return [any(why[s] for s in range(4 * k, min(4 * k + 4, len(why)))) for k in range(geometry(case).groups)]


def strip_wide_mask(case, src):
    """(h, w) bool: the sample lies in a strip of a wide group."""
    g = geometry(case)
    gw = group_wide(case, src)
    m = np.zeros((case.h, case.w), bool)
    for s in range(g.strips):
        y0, x0 = strip_origin(case, s)
        m[y0:y0 + case.ctb, x0:x0 + g.sw] = gw[s // 4]
    return m


# ------------------------------------------------------------------ references

@functools.lru_cache(maxsize=None)
def _reference(case, kind, qp, closed, pid, luma):
    src = source(case, kind)
    fn = O.tu_pipeline_plane_closed if closed else O.tu_pipeline_plane
    return tuple(_ro(a) for a in fn(src, case.ctb, pid, case.seed, qp, luma))


def source(case, kind):
    """Plane ``kind``: a .. e, a name of ``plants`` (that single-plant plane) or such a name + "!" (the plant
    with the value FAR)."""
    if len(kind) == 1:
        return plane(case, kind)
    return plane_c_single(case, kind.rstrip("!"), FAR if kind.endswith("!") else None)


def reference(case, kind, qp, closed=False, pid=None, luma=None):
    """The oracle's read-only (levels, recon, TU map) of plane ``kind`` (see ``source``) of the case."""
    return _reference(case, kind, int(qp), bool(closed), plane_id(case) if pid is None else pid,
                      case.luma if luma is None else bool(luma))


def tu_map(case, pid=None):
    """The TU map: a function of (ctb, plane id, seed, w, h) only."""
    return reference(case, "a", case.qp, pid=pid)[2]


def tu_of(tu, y, x):
    """(x0, y0, N) of the TU that holds sample (y, x) under the map ``tu``."""
    n = 1 << int(tu[y // 4, x // 4])
    return x - x % n, y - y % n, n


def describe(case, name, got, want, tu, at=(0, 0)):
    """None when equal; else the case, the output, the first differing sample and its TU.  ``tu``: the
    plane's TU map; ``at``: the plane position (y, x) of element (0, 0) of the arrays compared."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{case.name}: {name}: shape / dtype {got.shape} {got.dtype}, want {want.shape} {want.dtype}"
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    y, x = (int(v) for v in bad[0])
    if name == "tu":
        y, x = 4 * y, 4 * x
    y, x = y + at[0], x + at[1]
    x0, y0, n = tu_of(tu, y, x)
    return (f"{case.name}: {name} differs at {len(bad)} of {want.size} elements, first at sample (y {y}, x {x}) of the "
            f"{n}x{n} TU at (y {y0}, x {x0}), strip {strip_at(case, y, x)}, group {strip_at(case, y, x) // 4}: "
            f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


# ------------------------------------------------------------------ census

Census = collections.namedtuple("Census", "origins outcomes")


@functools.lru_cache(maxsize=None)
def census(case):
    """origins[group][k]: TU origins of size 4 << k in the group (whole-plane call).
    outcomes[kind][k]: [TUs where DC wins strictly, where planar wins strictly, ties] at size 4 << k on plane
    ``kind``, open loop: neighbours from the source, 128 at the border (DC is coded on a tie)."""
    tu = tu_map(case)
    assert R.valid(tu, case.ctb)
    list_ = R.tus(tu, case.ctb)
    origins = np.zeros((geometry(case).groups, 4), np.int64)
    for x, y, n in list_:
        origins[strip_at(case, y, x) // 4, int(np.log2(n)) - 2] += 1
    outcomes = {}
    for kind in KINDS_8BIT + KINDS_WIDE:
        src = plane(case, kind)
        pm = R.pred_map(src, src, tu, case.ctb)
        cnt = np.zeros((4, 3), np.int64)
        for x, y, n in list_:
            e_dc, e_pl = R.pred_energies(src, src, x, y, n)
            assert int(pm[y // 4, x // 4]) == (1 if e_dc <= e_pl else 0)
            cnt[int(np.log2(n)) - 2, 0 if e_dc < e_pl else 1 if e_pl < e_dc else 2] += 1
        outcomes[kind] = _ro(cnt)
    return Census(_ro(origins), outcomes)


def sizes(case):
    return [n for n in (4, 8, 16, 32) if n <= case.ctb]


def batch_unit(n):
    """TUs per batch of the open-loop kernel: 64 / N lanes-per-TU; 32 x 32 TUs on the packed butterflies run
    two per batch (one per wave on the matrix cores: a trailing batch is then never partial)."""
    return 64 // n


# ------------------------------------------------------------------ padded layouts

Layout = collections.namedtuple("Layout", "base pitch plane_stride group_stride size")


def layout(case, base, pitch, ppg, groups, gap=0):
    """``groups`` groups of ``ppg`` planes one behind the other, ``gap`` elements between planes."""
    ps = case.h * pitch + gap
    return Layout(base, pitch, ps, ppg * ps, base + groups * ppg * ps)


def plane_offsets(lay, ppg, groups):
    return [lay.base + g * lay.group_stride + c * lay.plane_stride for g in range(groups) for c in range(ppg)]


def view(buf, case, lay, off):
    """Writable (h, w) view of the plane at element ``off`` of the 1-D array ``buf``."""
    return np.lib.stride_tricks.as_strided(buf[off:], (case.h, case.w), (lay.pitch * buf.itemsize, buf.itemsize))


def fill(case, lay, planes_, offs, pad_value=SENTINEL):
    """The source buffer: ``pad_value`` outside the planes."""
    buf = np.full(lay.size, pad_value, np.int16)
    for p, off in zip(planes_, offs):
        view(buf, case, lay, off)[:] = p
    return buf


def outside_mask(case, lay, offs):
    m = np.ones(lay.size, bool)
    for off in offs:
        view(m, case, lay, off)[:] = False
    return m
