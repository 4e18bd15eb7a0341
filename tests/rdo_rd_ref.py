"""Test helper: the 35-mode intra RDO with a rate term per full NxN block (DESIGN.md
§3.3b open loop, §3.7b closed loop) restated on the CPU from the pinned oracle's
primitives only -- what ``gpu.intra_rdo_rd_planes_n`` / ``gpu.intra_rdo_rd_closed_n``
are compared with.  Per mode the unchanged chain of rdo_ref.chain, D = its SSE,
R = count_nonzero(level) + 1, J = D + lam * R in Python integers; the lowest J wins,
ties go to the lowest mode.  At lam = 0 it equals rdo_ref.rdo_plane /
rdo_closed_ref.rdo_plane_closed, and it reproduces the reference-composed records of
tests/golden/rdo_rd.npz bit-exactly: test_rdo_rd_host.py."""
import numpy as np

import rdo_closed_ref
import rdo_ref
from rdo_ref import chain

# The lambdas of the tests, per kind (n, use_dst): (picture is wide, qp, lam).  At these the
# mode map differs from lam = 0's in >= 3 of 9 blocks of the (3N+2) x (3N+3) pictures, both loops.
TABLE = {(4, True): (False, 22, 1000), (4, False): (False, 22, 1000), (8, False): (False, 4, 10 ** 4),
         (16, False): (True, 4, 10 ** 7), (32, False): (True, 4, 10 ** 7)}
KINDS = list(TABLE)
LAM_MAX = 2 ** 31 - 1


def table_picture(n, use_dst, h=None, w=None):
    """The picture of kind (n, use_dst) at (3N+2) x (3N+3) (or h x w): seed 1000 + N + dst."""
    h, w = h or 3 * n + 2, w or 3 * n + 3
    seed = 1000 + n + int(use_dst)
    return rdo_closed_ref.wide_picture(h, w, seed) if TABLE[(n, bool(use_dst))][0] else rdo_ref.picture(h, w, seed)


def _walk(src, n, qp, lam, use_dst, closed, lvl, rec):
    src = np.ascontiguousarray(src, np.int16)
    h, w = src.shape
    lam = int(lam)
    modes = np.zeros((h // n, w // n), np.uint8)
    tied = np.zeros((h // n, w // n), bool)
    work = np.zeros(src.shape, np.int16)          # closed loop: Plane.zeros, what the neighbour fetch reads
    sj = sd = sr = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            orig = np.ascontiguousarray(src[by:by + n, bx:bx + n])
            best, js = None, []
            for m in range(35):
                pred = rdo_closed_ref.predict(work, bx, by, n, m) if closed else rdo_ref.predict(src, bx, by, n, m)
                l, r, d = chain(orig, pred, qp, n, use_dst)
                rate = int(np.count_nonzero(l)) + 1
                j = d + lam * rate
                js.append(j)
                if best is None or j < best[0]:   # ties: the lowest mode
                    best = (j, m, l, r, d, rate)
            sj, sd, sr = sj + best[0], sd + best[4], sr + best[5]
            modes[by // n, bx // n] = best[1]
            tied[by // n, bx // n] = js.count(best[0]) > 1
            lvl[by:by + n, bx:bx + n] = best[2]
            (work if closed else rec)[by:by + n, bx:bx + n] = best[3]
    if closed:
        rec[:] = work
    return modes, lvl, rec, (sj, sd, sr), tied


def rd_plane(src, n, qp, lam, use_dst=False, lvl=None, rec=None):
    """Open loop: (modes (h/n, w/n) uint8, lvl int32, rec int16, (sum J, sum D, sum R), tied bool map).
    ``lvl`` / ``rec`` given: written in place, samples outside full blocks untouched."""
    lvl = np.zeros(np.shape(src), np.int32) if lvl is None else lvl
    rec = np.zeros(np.shape(src), np.int16) if rec is None else rec
    return _walk(src, n, qp, lam, use_dst, False, lvl, rec)


def rd_plane_closed(src, n, qp, lam, use_dst=False, lvl=None, rec=None):
    """Closed loop: the same tuple.  ``lvl`` given: written in place, samples outside full blocks
    untouched; ``rec`` given: overwritten whole (0 outside full blocks)."""
    lvl = np.zeros(np.shape(src), np.int32) if lvl is None else lvl
    rec = np.zeros(np.shape(src), np.int16) if rec is None else rec
    return _walk(src, n, qp, lam, use_dst, True, lvl, rec)
