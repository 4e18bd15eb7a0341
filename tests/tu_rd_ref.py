"""Test helper: config 4 with a chosen or a supplied quadtree, open loop (DESIGN.md
§3.4a), restated on the CPU from the pinned oracle's primitives only -- what
``gpu.tu_rd_planes`` and ``gpu.tu_encode_map_planes`` are compared with.
``rd_plane`` reproduces the reference-composed records of tests/golden/tu_rd.npz and
``encode_map`` on a seeded map reproduces ``O.tu_pipeline_plane``: test_tu_rd_host.py."""
import numpy as np

from oracle import oracle as O

import tu_decode_ref as R

QP_LAMBDA = [(22, 0), (22, 400), (22, 3000), (32, 1000)]   # the (qp, lambda) pairs of the mixed fixture


def mixed_picture(h, w):
    """The mixed fixture: a flat quarter, a flat quarter with sparse impulses, a noisy
    wave and a ramp -- every TU size wins somewhere at the pairs of QP_LAMBDA."""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(11)
    a = np.full((h, w), 90.0)
    a[h // 2:, :] = (128 + 60 * np.sin(x / 5 + y / 9))[h // 2:, :] + rng.integers(-6, 7, (h - h // 2, w))
    a[:h // 2, w // 2:] += rng.integers(-30, 31, (h // 2, w - w // 2)) * (rng.random((h // 2, w - w // 2)) < 0.02)
    a[h // 2:, w // 2:] = (40 + 1.0 * x + 0.5 * y)[h // 2:, w // 2:]
    return a.clip(0, 255).astype(np.int16)


def neighbours(src, x, y, n):
    """n source samples above and to the left, 128 outside the plane (D12)."""
    top = np.full(n, 128, np.int16) if y == 0 else src[y - 1, x:x + n].copy()
    left = np.full(n, 128, np.int16) if x == 0 else src[y:y + n, x - 1].copy()
    return top, left


def energy(res):
    return int((res.astype(np.int64) ** 2).sum())


def tu_chain(src, x, y, n, qp, is_luma):
    """§3.4's chain on the TU (x, y, n): (lvl int32, rec int16, dc 0 / 1, D, R)."""
    orig = np.ascontiguousarray(src[y:y + n, x:x + n])
    top, left = neighbours(src, x, y, n)
    dc, pl = O.intra_dc(top, left, n), O.intra_planar(top, left, int(top[-1]), int(left[-1]), n)
    use_dc = energy(O.residual(orig, dc)) <= energy(O.residual(orig, pl))   # DC wins ties
    pred = dc if use_dc else pl
    dst = bool(is_luma) and n == 4
    lvl = O.quantize(O.forward_transform(O.residual(orig, pred), dst), qp, n)
    rres = O.inverse_transform(O.dequantize(lvl, qp), dst)
    rec = O.clip(O.reconstruct(pred, rres.astype(np.int16)), 8)
    return lvl, rec, int(use_dc), energy(O.residual(orig, rec)), int(np.count_nonzero(lvl)) + 1


class Chains:
    """Per-TU results of one plane, computed on first use."""

    def __init__(self, src, qp, is_luma):
        self.src, self.qp, self.is_luma = np.ascontiguousarray(src, np.int16), qp, is_luma
        self.c = {}

    def __call__(self, x, y, n):
        k = (x, y, n)
        if k not in self.c:
            self.c[k] = tu_chain(self.src, x, y, n, self.qp, self.is_luma)
        return self.c[k]


def rd_plane(src, ctb, qp, lam, is_luma, parent_wins=lambda j, kids: j <= kids, chains=None, per_ctb=None):
    """The search: (tu, pm uint8 (h/4, w/4), lvl int32, rec int16, stats int64 [J, D, R]).
    ``parent_wins`` replaces the decision rule: only for tests that show their inputs
    tell the rule from a variant of it.  ``per_ctb`` (a dict) receives J per CTB origin."""
    src = np.ascontiguousarray(src, np.int16)
    h, w = src.shape
    ch = chains or Chains(src, qp, is_luma)
    tu = np.zeros((h // 4, w // 4), np.uint8)
    pm = np.zeros((h // 4, w // 4), np.uint8)
    lvl = np.zeros((h, w), np.int32)
    rec = np.zeros((h, w), np.int16)
    tot = np.zeros(3, np.int64)

    def best(x, y, s):
        """(J, [TUs]) of the node."""
        if x >= w or y >= h:
            return 0, []
        inside = x + s <= w and y + s <= h
        if s == 4:
            _, _, _, d, r = ch(x, y, 4)
            return d + lam * r, [(x, y, 4)]
        kids, tus = 0, []
        for dy in (0, s // 2):
            for dx in (0, s // 2):
                j, t = best(x + dx, y + dy, s // 2)
                kids += j
                tus += t
        if inside:
            _, _, _, d, r = ch(x, y, s)
            if parent_wins(d + lam * r, kids):
                return d + lam * r, [(x, y, s)]
        return kids, tus

    for cy in range(0, h, ctb):
        for cx in range(0, w, ctb):
            j, tus = best(cx, cy, ctb)
            if per_ctb is not None:
                per_ctb[(cx, cy)] = j
            for x, y, n in tus:
                l, r, m, d, rate = ch(x, y, n)
                lvl[y:y + n, x:x + n] = l
                rec[y:y + n, x:x + n] = r
                tu[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = int(np.log2(n))
                pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = m
                tot += (d + lam * rate, d, rate)
    return tu, pm, lvl, rec, tot


def encode_map(src, tu, ctb, qp, lam, is_luma, chains=None):
    """The map-driven encode of a valid map: (pm, lvl, rec, stats)."""
    src = np.ascontiguousarray(src, np.int16)
    ch = chains or Chains(src, qp, is_luma)
    pm = np.zeros(np.asarray(tu).shape, np.uint8)
    lvl = np.zeros(src.shape, np.int32)
    rec = np.zeros(src.shape, np.int16)
    tot = np.zeros(3, np.int64)
    for x, y, n in R.tus(tu, ctb):
        l, r, m, d, rate = ch(x, y, n)
        lvl[y:y + n, x:x + n] = l
        rec[y:y + n, x:x + n] = r
        pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = m
        tot += (d + lam * rate, d, rate)
    return pm, lvl, rec, tot


def area_shares(tu, ctb):
    """Share of the plane's area per admissible TU size, smallest first."""
    tu = np.asarray(tu)
    return [float((tu == v).mean()) for v in range(2, int(np.log2(ctb)) + 1)]
