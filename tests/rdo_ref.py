"""Test helper: the 35-mode open-loop intra RDO per full NxN block (DESIGN.md
§3.3a) restated on the CPU from the pinned oracle's primitives only -- what
``gpu.intra_rdo_planes_n`` is compared with.  At N = 8 it equals
``O.intra_rdo_plane``, and it reproduces the reference-composed records of
tests/golden/rdo_n.npz bit-exactly: test_rdo_n_host.py."""
import numpy as np

from oracle import oracle as O


def picture(h, w, seed):
    """The 8-bit test picture of the RDO tests: smooth waves + noise, one quadrant posterised."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = (128 + 60 * np.sin(x / 5 + y / 9) + 40 * np.cos(y / 3 - x / 11) + rng.integers(-6, 7, (h, w))).clip(0, 255)
    a[h // 2:, w // 3:] = (a[h // 2:, w // 3:] // 32) * 32
    return a.astype(np.int16)


def neighbors(src, x, y, count):
    """BlockView.get_top/left_neighbors(count), get_top_left_neighbor (block.py:38-55):
    128 outside the plane, numpy slice truncation at the right / bottom edge."""
    top = np.full(count, 128, np.int16) if y == 0 else src[y - 1, x:x + count].copy()
    left = np.full(count, 128, np.int16) if x == 0 else src[y:y + count, x - 1].copy()
    tl = 128 if (y == 0 or x == 0) else int(src[y - 1, x - 1])
    return top, left, tl


def predict(src, x, y, n, mode):
    top, left, tl = neighbors(src, x, y, n)
    if mode == 0:
        return O.intra_planar(top, left, int(top[-1]), int(left[-1]), n)
    if mode == 1:
        return O.intra_dc(top, left, n)
    top2, left2, _ = neighbors(src, x, y, 2 * n)
    return O.intra_angular(np.concatenate([[tl], top2]), np.concatenate([[tl], left2]), tl, mode, n)


def chain(orig, pred, qp, n, use_dst):
    lvl = O.quantize(O.forward_transform(O.residual(orig, pred), use_dst), qp, n)
    rres = O.inverse_transform(O.dequantize(lvl, qp), use_dst)
    rec = O.clip(O.reconstruct(pred, rres.astype(np.int16)), 8)
    sse = int(np.sum(O.residual(orig, rec).astype(np.int64) ** 2))
    return lvl, rec, sse


def rdo_plane(src, n, qp, use_dst=False, lvl=None, rec=None):
    """(modes (h/n, w/n) uint8, lvl int32, rec int16, sse int) of one plane; ``lvl`` / ``rec``
    given: written in place, samples outside full blocks untouched."""
    src = np.ascontiguousarray(src, np.int16)
    h, w = src.shape
    modes = np.zeros((h // n, w // n), np.uint8)
    lvl = np.zeros(src.shape, np.int32) if lvl is None else lvl
    rec = np.zeros(src.shape, np.int16) if rec is None else rec
    total = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            orig = np.ascontiguousarray(src[by:by + n, bx:bx + n])
            best = None
            for m in range(35):
                l, r, sse = chain(orig, predict(src, bx, by, n, m), qp, n, use_dst)
                if best is None or sse < best[0]:      # ties: the lowest mode
                    best = (sse, m, l, r)
            total += best[0]
            modes[by // n, bx // n] = best[1]
            lvl[by:by + n, bx:bx + n] = best[2]
            rec[by:by + n, bx:bx + n] = best[3]
    return modes, lvl, rec, total


def has_tie(src, n, qp, use_dst=False):
    """True when some block's lowest cost is reached by more than one mode."""
    src = np.ascontiguousarray(src, np.int16)
    h, w = src.shape
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            orig = np.ascontiguousarray(src[by:by + n, bx:bx + n])
            costs = [chain(orig, predict(src, bx, by, n, m), qp, n, use_dst)[2] for m in range(35)]
            if costs.count(min(costs)) > 1:
                return True
    return False
