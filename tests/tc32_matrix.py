"""Test helper: config 5 (tc32_plane, tc32_planes, tc32_planes_compact,
tc32_levels_widen) over its block pairings, its wide rule, its level bound and its layouts.  CPU only,
built on the pinned oracle and tu_decode_ref.py; test_tc32_matrix_host.py checks the conditions below
with the oracle alone, test_tc32_matrix_gpu.py runs the cases on the GPU.

Block order (``wave_of``, ``wave_pairs``).  These restate the DEFAULT form of k_tc32_hd (nh_ctu.hip,
k_tc32_hd<2, LT, ILV = true>, 4 waves per workgroup): the full 32 x 32 blocks of a plane are numbered in
raster order, workgroup g holds blocks 8 g .. 8 g + 7 and its wave w codes block 8 g + w and then block
8 g + w + 4; the wait before the second block depends on whether the first was narrow or wide.  They
MUST follow the kernel if that order changes.

Geometry cases, by (blocks across, blocks down): 1 x 1, 1 x 9 (one column), 9 x 1, 2 x 3, 5 x 2 and
11 x 2 (the PAIRING case); each but 1 x 1 with a ragged right and bottom edge.  Between them: workgroups
of exactly 8 blocks, a workgroup whose waves hold two blocks or one (5 .. 7 blocks), workgroups whose
waves hold one block or none (1 .. 3 blocks) and wave pairs in two block rows.  A workgroup with waves
of two blocks, of one AND of none cannot exist under this order: wave w has two blocks only when block
8 g + w + 4 exists, and then every block 8 g .. 8 g + 3 exists, so every wave has at least one.

Planes of a case (all int16):
  a  8-bit gradient + noise;
  b  samples 0 / 255 only;
  c  plane a with every wide sample of ``plants``;
  d  full-range int16 noise;
  e  8-bit noise with a patch of 128 over whole blocks at the top-left corner, and the TIE block;
  f  a checkerboard of whole 32 x 32 blocks of 0 and 255: every interior block sees a DC prediction of
     255 - its own value and reaches level +51 / -51 at QP 0, the bound of the int8 compact levels.  Only
     a block with a block above it AND a block left of it reaches the bound (at the plane's border half
     the neighbours are 128): 1 x 1, 1 x 9 and 9 x 1 have none, their largest |level| is 25 / 38 / 38,
     and +51 / -51 is asserted on 2 x 3, 5 x 2 and 11 x 2 only.  Non-zero levels at QP 4 and QP 22 hold on
     every case;
  NAME / NAME!  plane a with the one plant NAME of ``plants``: the table's 9-bit value / ``FAR``.

DC against planar.  Config 5 writes no mode map, so a wrong choice shows only where the two predictions
differ.  On plane e's patch of 128 -- and on the top-left block of any plane, whose neighbours are all
128 -- they tie with IDENTICAL predictions: either choice gives the same outputs.  Plane e therefore
also holds a constructed tie (``tie_block``; not at 1 x 1, which has only the top-left block): top
neighbours t, left neighbours l = t - 64, so DC = c = (t + l) / 2 and planar = c + x - y; the block is
c above the diagonal and c + x - y below it, and the two residual energies are the same sum of
(x - y)^2.  At QP 51 every level is zero and the reconstruction is the chosen prediction itself.

A block is WIDE (``block_wide``, restated from the rule) when one of its own samples, of the 32 samples
above it or of the 32 samples left of it is outside 0..255 (128 outside the plane)."""
import collections
import functools

import numpy as np

import tu_decode_ref as R
from oracle import oracle as O
from tu_matrix import FAR, SENTINEL, Layout, plane_offsets, view  # noqa: F401  (these fit unchanged)

SENTINEL8 = 0x5A                # int8 levels: no level (|level| <= 51) and not the marker
MARK = {2: -32768, 1: -128}     # compact levels: a wide block's origin, by level size in bytes
MARK_REC = -32768               # what the narrow launch leaves at a wide block's recon origin for the fix-up

# patch: plane e's constant patch in blocks (columns, rows); tie: the constructed tie block (bx, by) or None
Case = collections.namedtuple("Case", "name nbx nby w h seed patch tie")


def _case(nbx, nby, w, h, seed, patch, tie):
    return Case(f"{nbx}x{nby}", nbx, nby, w, h, seed, patch, tie)


# sizes and seeds found on the CPU (test_tc32_matrix_host.py asserts every condition)
CASES = (
    _case(1, 1, 32, 32, 5, (0, 0), None),
    _case(1, 9, 40, 300, 5, (1, 1), (0, 2)),
    _case(9, 1, 296, 44, 5, (1, 1), (2, 0)),
    _case(2, 3, 76, 100, 5, (1, 1), (1, 1)),
    _case(5, 2, 172, 72, 5, (1, 1), (2, 1)),
    _case(11, 2, 360, 76, 5, (2, 1), (6, 1)),
)
BY_NAME = {c.name: c for c in CASES}
PAIRING = BY_NAME["11x2"]
QPS = (0, 4, 22, 51)            # on the 8-bit planes
QPS_INT16 = (3, 51)             # on plane d
KINDS_8BIT = ("a", "b", "e", "f")
KINDS_WIDE = ("c", "d")
KINDS = ("a", "b", "c", "d", "e", "f")


def nblk(case):
    return case.nbx * case.nby


def block_origin(case, b):
    return (b // case.nbx) * 32, (b % case.nbx) * 32        # (y, x)


def block_at(case, y, x):
    """Index of the full block that holds sample (y, x); None in the partial column / row."""
    if y >= 32 * case.nby or x >= 32 * case.nbx:
        return None
    return (y // 32) * case.nbx + x // 32


def wave_of(b):
    """(workgroup, wave, 0 = the wave's first block / 1 = its second) of block ``b``."""
    return b // 8, b % 4, (b % 8) // 4


def wave_pairs(n):
    """Per wave that has a block, in (workgroup, wave) order: (first block, second block or None)."""
    out = []
    for g in range(-(-n // 8)):
        for w in range(4):
            b = 8 * g + w
            if b < n:
                out.append((b, b + 4 if b + 4 < n else None))
    return out


# ------------------------------------------------------------------ planes

def _ro(a):
    a.setflags(write=False)
    return a


def _rng(case, salt):
    return np.random.default_rng([case.seed, case.nbx, case.nby, salt])


def tie_params(case):
    """(t, l, c) of the tie block: its top neighbours, its left neighbours (128 at the plane's border)
    and the DC prediction."""
    bx, by = case.tie
    t, l = (128, 64) if by == 0 else (192, 128) if bx == 0 else (160, 96)
    return t, l, (t + l) // 2


@functools.lru_cache(maxsize=None)
def plane(case, kind):
    """Read-only plane ``kind`` (a .. f) of the case."""
    h, w = case.h, case.w
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "a":
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
    if kind == "f":
        return _ro((((xx // 32 + yy // 32) % 2) * 255).astype(np.int16))
    assert kind == "e"
    p = _rng(case, 5).integers(0, 256, (h, w)).astype(np.int16)
    p[:case.patch[1] * 32, :case.patch[0] * 32] = 128
    if case.tie:
        bx, by = case.tie
        t, l, c = tie_params(case)
        y0, x0 = 32 * by, 32 * bx
        if by:
            p[y0 - 1, x0:x0 + 32] = t
        if bx:
            p[y0:y0 + 32, x0 - 1] = l
        d = xx[:32, :32] - yy[:32, :32]
        p[y0:y0 + 32, x0:x0 + 32] = c + np.minimum(d, 0)
    return _ro(p)


@functools.lru_cache(maxsize=None)
def plants(case):
    """name -> (y, x, value) of plane c's wide samples, 9-bit positive and negative values; a plant is left
    out where the case has no place for it (one block column, one block row, no ragged edge)."""
    nbx, nby = case.nbx, case.nby
    out = {}
    x0 = 32 * min(5, nbx - 1)
    out["interior"] = (13, x0 + 17, 300)
    if nbx >= 2:
        out["right_edge"] = (7, 31, -1)                         # block 0's last column
    if nby >= 2:
        out["bottom_edge"] = (31, 32 * min(9, nbx - 1) + 5, 256)   # last row of a block of block row 0
    if nbx >= 2 and nby >= 2:
        out["corner_br"] = (31, 32 * min(2, nbx - 2) + 31, 511)    # bottom-right corner sample of block UL
        out["corner_bl"] = (31, 32 * max(1, min(8, nbx - 1)), -256)   # bottom-left corner sample of block UR
    out["last"] = (32 * nby - 1, 32 * nbx - 1, -300)
    if case.w % 32:
        out["partial_col"] = (32 * nby - 2, 32 * nbx, 400)
    if case.h % 32:
        out["partial_row"] = (32 * nby, 32 * nbx - 2, -2)
    assert len({(y, x) for y, x, _ in out.values()}) == len(out)
    return out


def plant_blocks(case, name):
    """block -> set of reasons ('own', 'top', 'left') the plant ``name`` alone turns it wide; ``narrow``:
    the blocks next to it that it must leave narrow.  Written per plant, independently of ``block_wide``."""
    y, x, _ = plants(case)[name]
    nbx = case.nbx
    if name in ("partial_col", "partial_row"):
        return {}, set(range(nblk(case)))
    b = (y // 32) * nbx + x // 32
    if name in ("interior", "last"):
        return {b: {"own"}}, set()
    if name == "right_edge":
        return {b: {"own"}, b + 1: {"left"}}, set()
    if name == "bottom_edge":
        return {b: {"own"}, b + nbx: {"top"}}, set()
    if name == "corner_br":
        return {b: {"own"}, b + 1: {"left"}, b + nbx: {"top"}}, {b + nbx + 1}
    assert name == "corner_bl"
    return {b: {"own"}, b + nbx: {"top"}}, {b - 1, b + nbx - 1}


def single_kinds(case):
    """The single-plant plane kinds of the case: NAME and NAME! for every plant."""
    return tuple(k for name in plants(case) for k in (name, name + "!"))


@functools.lru_cache(maxsize=None)
def source(case, kind):
    """Plane ``kind``: a .. f, a name of ``plants`` (plane a with that plant alone) or such a name + "!" (the
    plant with the value FAR)."""
    if len(kind) == 1:
        return plane(case, kind)
    p = plane(case, "a").copy()
    y, x, v = plants(case)[kind.rstrip("!")]
    p[y, x] = FAR if kind.endswith("!") else v
    return _ro(p)


# ------------------------------------------------------------------ the wide rule

def _wide(a):
    a = np.asarray(a)
    return bool(((a < 0) | (a > 255)).any())


def block_reasons(case, src):
    """Per full block the set of reasons it is wide: 'own' (a sample of the block), 'top' (the row above it,
    over its own columns), 'left' (the column left of it, over its own rows); 128 outside the plane."""
    out = []
    for b in range(nblk(case)):
        y0, x0 = block_origin(case, b)
        why = set()
        if _wide(src[y0:y0 + 32, x0:x0 + 32]):
            why.add("own")
        if y0 > 0 and _wide(src[y0 - 1, x0:x0 + 32]):
            why.add("top")
        if x0 > 0 and _wide(src[y0:y0 + 32, x0 - 1]):
            why.add("left")
        out.append(why)
    return out


def block_wide(case, src):
    """Per full block: coded by the int8 fix-up (variant 1), marked in the compact levels."""
    return [bool(w) for w in block_reasons(case, src)]


def pairings(case, src):
    """The set of wave forms on the plane: 'nn', 'nw', 'wn', 'ww' (first block, second block of one wave),
    'n' / 'w' (a wave with one block)."""
    wide = block_wide(case, src)
    return {"".join("w" if wide[b] else "n" for b in pair if b is not None) for pair in wave_pairs(nblk(case))}


def workgroup_wide(case, src):
    wide = block_wide(case, src)
    return [any(wide[8 * g:8 * g + 8]) for g in range(-(-nblk(case) // 8))]


# ------------------------------------------------------------------ references

@functools.lru_cache(maxsize=None)
def _reference(case, kind, qp):
    return tuple(_ro(a) for a in O.tc32_plane(source(case, kind), qp))


def reference(case, kind, qp):
    """The oracle's read-only (levels int32, recon int16) of plane ``kind`` (see ``source``); only the full
    blocks are specified (``full``)."""
    return _reference(case, kind, int(qp))


def full(case, a):
    """The full-block region of a plane-shaped array."""
    return a[:32 * case.nby, :32 * case.nbx]


def full_mask(case):
    m = np.zeros((case.h, case.w), bool)
    full(case, m)[:] = True
    return m


def describe(case, name, got, want, src, at=(0, 0)):
    """None when equal; else the case, the output, the count of differing elements, the first differing
    sample, its block, that block's (workgroup, wave, first / second block of the wave) and what the rule
    says of the block.  ``src``: the plane; ``at``: the plane position (y, x) of element (0, 0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{case.name}: {name}: shape / dtype {got.shape} {got.dtype}, want {want.shape} {want.dtype}"
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    y, x = (int(v) + o for v, o in zip(bad[0], at))
    b = block_at(case, y, x)
    where = "outside the full blocks"
    if b is not None:
        g, w, k = wave_of(b)
        where = (f"block {b} (workgroup {g}, wave {w}, its {'second' if k else 'first'} block; "
                 f"{'wide' if block_wide(case, src)[b] else 'narrow'} by the rule)")
    return (f"{case.name}: {name} differs at {len(bad)} of {want.size} elements, first at sample (y {y}, x {x}) of "
            f"{where}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


# ------------------------------------------------------------------ census

@functools.lru_cache(maxsize=None)
def census(case, kind):
    """Per full block of plane ``kind``: (e_dc, e_planar), open loop: neighbours from the source, 128 at the
    border (DC is coded on a tie)."""
    src = source(case, kind)
    return tuple(R.pred_energies(src, src, *block_origin(case, b)[::-1], 32) for b in range(nblk(case)))


def outcomes(case, kind):
    """[blocks where DC wins strictly, where planar wins strictly, ties]."""
    e = census(case, kind)
    return [sum(a < b for a, b in e), sum(b < a for a, b in e), sum(a == b for a, b in e)]


def predictions(case, kind, b):
    """(DC, planar) prediction of block ``b``, open loop."""
    src = source(case, kind)
    y, x = block_origin(case, b)
    return R._preds(src, x, y, 32)


# ------------------------------------------------------------------ padded layouts

def layout(case, base, pitch, ppg, groups, gap=0, group_gap=0):
    """``groups`` groups of ``ppg`` planes one behind the other, ``gap`` elements behind every plane and
    ``group_gap`` more behind every group; ``tail`` = gap + group_gap elements end the buffer."""
    ps = case.h * pitch + gap
    gs = ppg * ps + group_gap
    return Layout(base, pitch, ps, gs, base + groups * gs)


def outside_full_mask(case, lay, offs):
    """True at every element of the buffer outside the planes' full blocks: before the base, pitch padding,
    gaps, partial blocks and the tail."""
    m = np.ones(lay.size, bool)
    for off in offs:
        full(case, view(m, case, lay, off))[:] = False
    return m


def wide_full_mask(case, lay, offs, kinds):
    """True at every element of a wide full block (where the spill plane is specified)."""
    m = np.zeros(lay.size, bool)
    for off, kind in zip(offs, kinds):
        v = view(m, case, lay, off)
        for b, w in enumerate(block_wide(case, source(case, kind))):
            if w:
                y0, x0 = block_origin(case, b)
                v[y0:y0 + 32, x0:x0 + 32] = True
    return m
