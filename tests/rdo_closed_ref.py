"""Test helper: the 35-mode CLOSED-loop intra RDO per full NxN block (DESIGN.md
§3.7a) restated on the CPU from the pinned oracle's primitives only -- what
``gpu.intra_rdo_closed_n`` is compared with.  Blocks in raster order on a
zero-initialised recon plane; every neighbour comes from the reconstruction
built so far.  At N = 8 it equals ``O.intra_rdo_plane(..., closed=True)``, and it
reproduces the reference-composed records of tests/golden/rdo_closed_n.npz
bit-exactly: test_rdo_closed_n_host.py."""
import numpy as np

from oracle import oracle as O
from rdo_ref import chain, neighbors, picture  # noqa: F401  (picture: re-exported for the tests)


def wide_picture(h, w, seed):
    """``picture`` stretched to about +-4000 around 128: at N = 32 an 8-bit source quantises to
    nothing at every QP, so the 32x32 tests need more than 8 bits."""
    return ((picture(h, w, seed).astype(np.int32) - 128) * 32 + 128).astype(np.int16)


def predict(rec, x, y, n, mode):
    """Mode ``mode`` of the block at (x, y) with neighbours from the reconstruction ``rec``."""
    top, left, tl = neighbors(rec, x, y, n)
    if mode == 0:
        return O.intra_planar(top, left, int(top[-1]), int(left[-1]), n)
    if mode == 1:
        return O.intra_dc(top, left, n)
    top2, _, _ = neighbors(rec, x, y, 2 * n)      # truncated at the right edge; past the last full block: 0
    topa = np.concatenate([[tl], top2]).astype(np.int16)
    lefta = np.concatenate([[tl], left]).astype(np.int16)      # the N reconstructed samples only
    return O.intra_angular(topa, lefta, tl, mode, n)


def _costs(orig, rec, x, y, n, qp, use_dst):
    """Per mode (levels, recon, sse) of the block at (x, y) with neighbours from ``rec``."""
    return [chain(orig, predict(rec, x, y, n, m), qp, n, use_dst) for m in range(35)]


def _walk(src, n, qp, use_dst, lvl, rec):
    src = np.ascontiguousarray(src, np.int16)
    h, w = src.shape
    modes = np.zeros((h // n, w // n), np.uint8)
    tied = np.zeros((h // n, w // n), bool)
    work = np.zeros(src.shape, np.int16)          # Plane.zeros: what the neighbour fetch reads
    total = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            orig = np.ascontiguousarray(src[by:by + n, bx:bx + n])
            res = _costs(orig, work, bx, by, n, qp, use_dst)
            sses = [r[2] for r in res]
            m = int(np.argmin(sses))              # ties: the lowest mode
            total += sses[m]
            modes[by // n, bx // n] = m
            tied[by // n, bx // n] = sses.count(sses[m]) > 1
            lvl[by:by + n, bx:bx + n] = res[m][0]
            work[by:by + n, bx:bx + n] = res[m][1]
    rec[:] = work
    return modes, lvl, rec, total, tied


def rdo_plane_closed(src, n, qp, use_dst=False, lvl=None, rec=None):
    """(modes (h/n, w/n) uint8, lvl int32, rec int16, sse int) of one plane.  ``lvl`` given: written in
    place, samples outside full blocks untouched; ``rec`` given: overwritten whole (0 outside full blocks)."""
    lvl = np.zeros(np.shape(src), np.int32) if lvl is None else lvl
    rec = np.zeros(np.shape(src), np.int16) if rec is None else rec
    return _walk(src, n, qp, use_dst, lvl, rec)[:4]


def tied_blocks(src, n, qp, use_dst=False):
    """Bool map (h/n, w/n): the block's lowest cost is reached by more than one mode."""
    return _walk(src, n, qp, use_dst, np.zeros(np.shape(src), np.int32), np.zeros(np.shape(src), np.int16))[4]


def has_tie(src, n, qp, use_dst=False):
    """True when some blocks of the plane are tied but not all of them."""
    t = tied_blocks(src, n, qp, use_dst)
    return bool(t.any() and not t.all())
