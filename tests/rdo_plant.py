"""Test helper: pictures on which EVERY one of the 35 intra modes is the RDO winner
(DESIGN.md §3.3a, §3.7a), for the five kinds N = 4 DST, 4 DCT, 8, 16, 32 in open and
in closed loop.  CPU only, built on the yardsticks rdo_ref.py / rdo_closed_ref.py and
the pinned oracle; test_rdo_plant_host.py checks it, test_rdo_modes_gpu.py uses it.

A. PLANTED winners.  A plane of 3 x 3 full blocks with ragged edges, (3N+1) x (3N+2).
   The source of one target block is overwritten with the yardstick's own prediction of
   mode m for that block (open loop: from the source neighbours; closed loop: from the
   reconstruction of the raster-earlier blocks, which do not depend on the target's
   source).  Mode m then has residual 0; every other mode pays for the distance between
   its prediction and m's.  A (picture seed, mode) pair counts as planted when
     1. mode m has the lowest cost of the target block,
     2. no other mode reaches that cost,
     3. the target's reference samples do not all hold one value,
   found by a seeded search over at most MAX_SEEDS pictures per mode.  Targets: block
   (1, 1) (interior: both references, a top-right and a below-left block), (1, 2) (last
   full block column: the top-right reference is truncated, or 0 past the last full block
   in closed loop) and (2, 1) (last full block row: the below-left reference is truncated
   in open loop).

B. CENSUS.  One noise plane of 16 x 32 blocks per recipe of CENSUS on which every mode
   wins at least one block with levels that are not all zero: the planted blocks have
   zero levels, so they do not show a winner's level store.

The references of the comparison are the yardsticks' plane functions at N != 8 and the
pinned oracle's ``intra_rdo_plane`` at N = 8."""
import functools

import numpy as np

import rdo_closed_ref
import rdo_ref
from oracle import oracle as O

SENTINEL = -12345
KINDS = ((4, True), (4, False), (8, False), (16, False), (32, False))     # (N, use_dst)
POSITIONS = ((1, 1), (1, 2), (2, 1))                                      # target (block row, block column)
MAX_SEEDS = 16

# Modes the search cannot plant within MAX_SEEDS pictures, (N, use_dst, closed, target) -> modes; every
# key not listed: none.  test_rdo_plant_host.py asserts that this is exactly what the search finds.
UNPLANTED = {(4, True, False, (2, 1)): (26, 27, 28), (4, False, False, (2, 1)): (26, 27, 28)}


def kind_name(n, dst, closed):
    return f"N = {n}{' DST' if dst else ' DCT' if n == 4 else ''}, {'closed' if closed else 'open'} loop"


def plane_shape(n):
    return 3 * n + 1, 3 * n + 2


def plant_qp(n):
    """The QPs of test_rdo_closed_n_gpu.py: at N = 32 only a fine quantiser codes anything (§3.7a)."""
    return 4 if n == 32 else 22


def plant_picture(n, closed, seed):
    """8-bit, but the wide picture at N = 32 in closed loop: an 8-bit one reconstructs to a constant 128
    there (§3.7a) and the references would be flat.  Open loop stays 8-bit at every N: the recon is clipped
    to 8 bits and a prediction from wide neighbours is not, so where the planted prediction lies outside
    0..255 (all of a wide DC block) the outputs no longer depend on it and an error of mode m would go
    unseen.  At N = 32 an 8-bit source quantises to nothing, recon = prediction: the planted block shows
    exactly the prediction and the winner's choice."""
    h, w = plane_shape(n)
    return rdo_closed_ref.wide_picture(h, w, seed) if (n == 32 and closed) else rdo_ref.picture(h, w, seed)


def plant_seed(k):
    """Picture seed of the search's step k.  The horizontal modes 9 and 10 are the rare ones: in closed
    loop at N = 8 the left block's coarse recon seldom leaves them apart, and of the seeds 0..119 only 16,
    30, 39, 51, 55, 67 and 91 plant them at (1, 1) (51 and 55 at (2, 1)); hence a window holding 51."""
    return 40 + k


def predict(plane, x, y, n, mode, closed):
    """The yardsticks' predictors, looked up at call time (test_rdo_plant_host.py patches them)."""
    return (rdo_closed_ref.predict if closed else rdo_ref.predict)(plane, x, y, n, mode)


def recon_before(src, n, qp, dst, pos):
    """rdo_closed_ref's walk stopped in front of block ``pos``: the plane its neighbours are read from."""
    h, w = src.shape
    work = np.zeros(src.shape, np.int16)
    for r in range(h // n):
        for c in range(w // n):
            if (r, c) == tuple(pos):
                return work
            orig = np.ascontiguousarray(src[r * n:(r + 1) * n, c * n:(c + 1) * n])
            res = [rdo_ref.chain(orig, predict(work, c * n, r * n, n, m, True), qp, n, dst) for m in range(35)]
            work[r * n:(r + 1) * n, c * n:(c + 1) * n] = res[int(np.argmin([x[2] for x in res]))][1]
    raise ValueError(f"no block {pos}")


def neighbour_plane(src, n, qp, dst, closed, pos):
    return recon_before(src, n, qp, dst, pos) if closed else src


def target_chains(src, nb, n, qp, dst, closed, pos):
    """Per mode (levels, recon, sse) of block ``pos`` of ``src`` with neighbours from ``nb``."""
    y, x = pos[0] * n, pos[1] * n
    orig = np.ascontiguousarray(src[y:y + n, x:x + n])
    return [rdo_ref.chain(orig, predict(nb, x, y, n, m, closed), qp, n, dst) for m in range(35)]


def target_outcome(chains):
    """(winner, levels, recon, sse) the yardsticks take from a block's per-mode chains: lowest cost, then
    lowest mode."""
    m = int(np.argmin([c[2] for c in chains]))
    return (m,) + tuple(chains[m])


def references_flat(nb, n, pos, closed):
    """The target's reference samples as the predictors fetch them (top-left, 2N top, 2N or -- closed loop --
    N left, truncated at the plane's edges) all hold one value."""
    top, left, tl = rdo_ref.neighbors(nb, pos[1] * n, pos[0] * n, 2 * n)
    return len(set(top.tolist()) | set(left[:n if closed else 2 * n].tolist()) | {tl}) == 1


def wins_alone(costs, m):
    return costs[m] == min(costs) and costs.count(costs[m]) == 1


@functools.lru_cache(maxsize=None)
def planted(n, dst, closed, pos):
    """{mode: (picture seed, read-only plane with mode planted at ``pos``)} for every mode the bounded
    search plants; each picture's neighbour plane and 35 predictions are shared by its modes."""
    qp = plant_qp(n)
    y, x = pos[0] * n, pos[1] * n
    found = {}
    for k in range(MAX_SEEDS):
        todo = [m for m in range(35) if m not in found]
        if not todo:
            break
        seed = plant_seed(k)
        pic = plant_picture(n, closed, seed)
        nb = neighbour_plane(pic, n, qp, dst, closed, pos)
        if references_flat(nb, n, pos, closed):
            continue
        preds = [predict(nb, x, y, n, m, closed) for m in range(35)]
        for m in todo:
            if wins_alone([rdo_ref.chain(preds[m], p, qp, n, dst)[2] for p in preds], m):
                src = pic.copy()
                src[y:y + n, x:x + n] = preds[m]
                src.setflags(write=False)
                found[m] = (seed, src)
    return found


# ------------------------------------------------------------------ plane sets and expected outputs

def layout(base, width, height, pitch, groups, group_stride):
    """One plane per group; the GPU test turns it into a ``gpu.plane_set``."""
    return dict(base=base, width=width, height=height, pitch=pitch, num_groups=groups, group_stride=group_stride)


def layout_end(s):
    return s["base"] + (s["num_groups"] - 1) * s["group_stride"] + (s["height"] - 1) * s["pitch"] + s["width"]


def plane_views(buf, sets):
    """Writable (h, w) views of every plane of the layouts ``sets`` inside the 1-D array ``buf``."""
    for s in sets:
        for g in range(s["num_groups"]):
            yield np.lib.stride_tricks.as_strided(buf[s["base"] + g * s["group_stride"]:], (s["height"], s["width"]),
                                                  (s["pitch"] * buf.itemsize, buf.itemsize))


def reference_plane(src, n, qp, dst, closed, lvl, rec):
    """(modes, sse) of one plane; levels and recon into the views ``lvl`` / ``rec`` as the entry points write
    them: full blocks only, but the closed loop's recon whole (0 outside full blocks).  N = 8: the pinned
    oracle; else the yardsticks."""
    if n != 8:
        fn = rdo_closed_ref.rdo_plane_closed if closed else rdo_ref.rdo_plane
        m, _, _, sse = fn(src, n, qp, dst, lvl=lvl, rec=rec)
        return m, sse
    m, l, r, sse = O.intra_rdo_plane(src, qp, closed=closed)
    fh, fw = src.shape[0] // 8 * 8, src.shape[1] // 8 * 8
    lvl[:fh, :fw] = l[:fh, :fw]
    if closed:
        rec[:] = r
    else:
        rec[:fh, :fw] = r[:fh, :fw]
    return m, sse


def expected(buf, sets, n, qp, dst, closed):
    """The reference over the layouts: (modes, lvl, rec, sse per plane), SENTINEL wherever nothing is written."""
    lvl = np.full(buf.shape, SENTINEL, np.int32)
    rec = np.full(buf.shape, SENTINEL, np.int16)
    modes, sse = [], []
    for s, lv, rv in zip(plane_views(buf, sets), plane_views(lvl, sets), plane_views(rec, sets)):
        m, t = reference_plane(np.ascontiguousarray(s), n, qp, dst, closed, lv, rv)
        modes.append(m.ravel())
        sse.append(t)
    return np.concatenate(modes), lvl, rec, np.array(sse, np.int64)


def locate(name, index, sets, n, want_modes):
    """Where element ``index`` of the output ``name`` (modes, lvl, rec or sse) lies: (plane number in set
    order or None, (y, x) in the plane or None, block (row, column) or None, the reference's winner of that
    block or None)."""
    k = mo = 0
    for s in sets:
        bh, bw = s["height"] // n, s["width"] // n
        for g in range(s["num_groups"]):
            if name == "sse" and index == k:
                return k, None, None, None
            if name == "modes" and mo <= index < mo + bh * bw:
                return k, None, divmod(index - mo, bw), int(want_modes[index])
            if name in ("lvl", "rec"):
                y, x = divmod(index - s["base"] - g * s["group_stride"], s["pitch"])
                if 0 <= y < s["height"] and x < s["width"]:
                    full = y < bh * n and x < bw * n
                    blk = (y // n, x // n) if full else None
                    return k, (y, x), blk, int(want_modes[mo + blk[0] * bw + blk[1]]) if full else None
            k += 1
            mo += bh * bw
    return None, None, None, None


def unspecified_levels(size, sets, n, closed):
    """Bool mask of the level elements whose contents the entry point leaves open: at N = 8 in closed loop
    (include/nanohevc.h), the samples of a plane outside its full blocks.  Elsewhere: none."""
    mask = np.zeros(size, bool)
    if n == 8 and closed:
        for v in plane_views(mask, sets):
            v[v.shape[0] // 8 * 8:] = True
            v[:, v.shape[1] // 8 * 8:] = True
    return mask


WIDE_SAMPLE = 300     # test_closed_wavefront_gpu.py's: one sample outside 0..255


def planted_launch(n, dst, closed, pos, wide=False):
    """One launch holding every planted mode of (kind, loop, target): (modes in plane order, buffer, layouts).
    The planted planes are the groups of one layout.  Targets (1, 1) and (2, 1): base, pitch and strides
    multiples of 8 (16-byte row stores); target (1, 2): an odd base, pitch = width + 3 and an odd gap
    between planes (element stores).  The gaps hold noise.  ``wide`` (N = 8): a second layout behind the
    first holds one 16 x 16 noise plane with a sample of WIDE_SAMPLE, which sends a closed-loop call to the
    32-bit form and that plane's group of an open-loop call to the general fallback launch."""
    found = planted(n, dst, closed, pos)
    modes = sorted(found)
    h, w = plane_shape(n)
    if pos == (1, 2):
        base, pitch = 5, w + 3
        stride = h * pitch + 7
    else:
        base, pitch = 8, (w + 7) // 8 * 8
        stride = h * pitch + 16
    sets = [layout(base, w, h, pitch, len(modes), stride)]
    if wide:
        sets.append(layout((layout_end(sets[0]) + 8 + 7) // 8 * 8, 16, 16, 16, 1, 256))
    rng = np.random.default_rng(40 + n)
    buf = rng.integers(0, 256, layout_end(sets[-1]) + 3).astype(np.int16)
    views = list(plane_views(buf, sets))
    for v, m in zip(views, modes):
        v[:] = found[m][1]
    if wide:
        views[-1][5, 6] = WIDE_SAMPLE
    return modes, buf, sets


# ------------------------------------------------------------------ census

# (N, use_dst, closed, noise amplitude, QP): uniform noise 0..255 (amplitude 255) or -amplitude..amplitude.
# 8-bit noise cannot make all 35 modes win in open loop at N = 8 (30-31 modes) or N = 16 (12): those
# recipes are wide, and there is no census of the packed open-loop form at N = 8 -- part A covers its modes.
CENSUS = ((4, True, False, 255, 10), (4, True, True, 255, 10), (4, False, False, 255, 10), (4, False, True, 255, 10),
          (8, False, False, 1000, 22), (8, False, True, 255, 10), (8, False, True, 1000, 22),
          (16, False, False, 4000, 10), (16, False, True, 4000, 10),
          (32, False, False, 4000, 10), (32, False, True, 4000, 10), (32, False, True, 4000, 22))
CENSUS_BLOCKS = (16, 32)     # block rows x block columns


def census_seed(n, dst):
    return 99 + n + dst


def census_plane(n, dst, amp):
    rng = np.random.default_rng(census_seed(n, dst))
    shape = (CENSUS_BLOCKS[0] * n, CENSUS_BLOCKS[1] * n)
    a = rng.integers(0, 256, shape) if amp == 255 else rng.integers(-amp, amp + 1, shape)
    return a.astype(np.int16)


@functools.lru_cache(maxsize=None)
def census(n, dst, closed, amp, qp):
    """(plane, layouts, expected outputs, per-mode count of blocks the mode wins with levels not all zero,
    share of the expected recon at 0 or 255); all read only."""
    src = census_plane(n, dst, amp)
    h, w = src.shape
    sets = [layout(0, w, h, w, 1, h * w)]
    want = expected(src.ravel(), sets, n, qp, dst, closed)
    modes, lvl, rec = want[0].reshape(CENSUS_BLOCKS), want[1].reshape(h, w), want[2]
    coded = np.abs(lvl).reshape(CENSUS_BLOCKS[0], n, CENSUS_BLOCKS[1], n).max(axis=(1, 3)) > 0
    counts = np.bincount(modes[coded].ravel(), minlength=35)
    for a in (src,) + want:
        a.setflags(write=False)
    return src, sets, want, counts, float(((rec == 0) | (rec == 255)).mean())
