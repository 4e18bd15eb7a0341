"""Generate tests/golden/tu_rd.npz by running the REFERENCE (build container only):

    python tests/golden/make_golden_tu_rd.py REFERENCE_DIR

The open-loop TU-size search of DESIGN.md §3.4a composed from the reference's own
functions: BlockView neighbours on the source plane, its DC / planar predictors,
transforms and quantizer, ``count_nonzero`` for the rate and ``residual_energy`` for
the DC-vs-planar choice and the distortion.  Four small 8-bit pictures: luma with
CTB 32 and chroma with CTB 16, two (qp, lambda) pairs each.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

# (ctb, is_luma, (h, w), qp, lambda)
CASES = [(32, True, (132, 164), 22, 400), (32, True, (132, 164), 32, 1000),
         (16, False, (68, 84), 22, 0), (16, False, (68, 84), 22, 3000)]


def picture(h, w):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(11)
    a = np.full((h, w), 90.0)
    a[h // 2:, :] = (128 + 60 * np.sin(x / 5 + y / 9))[h // 2:, :] + rng.integers(-6, 7, (h - h // 2, w))
    a[:h // 2, w // 2:] += rng.integers(-30, 31, (h // 2, w - w // 2)) * (rng.random((h // 2, w - w // 2)) < 0.02)
    a[h // 2:, w // 2:] = (40 + 1.0 * x + 0.5 * y)[h // 2:, w // 2:]
    return a.clip(0, 255).astype(np.int16)


def ref_tu(I, T, Q, M, plane, x, y, n, qp, is_luma):
    from nano_hevc.block import BlockView
    blk = BlockView(plane, x, y, n)
    orig = blk.copy_pixels()
    top, left = blk.get_top_neighbors(n), blk.get_left_neighbors(n)
    dc = I.intra_dc_predict(top, left, n)
    pl = I.intra_planar_predict(top, left, int(top[-1]), int(left[-1]), n)
    use_dc = M.residual_energy(I.residual_block(orig, dc)) <= M.residual_energy(I.residual_block(orig, pl))
    pred = dc if use_dc else pl
    dst = bool(is_luma) and n == 4
    lvl = Q.quantize_block(T.forward_transform(I.residual_block(orig, pred), use_dst=dst), qp)
    rres = T.inverse_transform(Q.dequantize_block(lvl, qp), use_dst=dst)
    rec = I.clip_to_pixel_range(I.reconstruct_block(pred, rres.astype(np.int16)), 8)
    d = int(M.residual_energy(I.residual_block(orig, rec)))
    return lvl, rec, int(use_dc), d, int(Q.count_nonzero(lvl)) + 1


def ref_rd_plane(I, T, Q, M, src, ctb, qp, lam, is_luma):
    from nano_hevc.frame import Plane
    plane = Plane(src.copy())
    h, w = src.shape
    cache = {}

    def tu_at(x, y, n):
        if (x, y, n) not in cache:
            cache[(x, y, n)] = ref_tu(I, T, Q, M, plane, x, y, n, qp, is_luma)
        return cache[(x, y, n)]

    def best(x, y, s):
        if x >= w or y >= h:
            return 0, []
        if s == 4:
            t = tu_at(x, y, 4)
            return t[3] + lam * t[4], [(x, y, 4)]
        kids, tus = 0, []
        for dy in (0, s // 2):
            for dx in (0, s // 2):
                j, t = best(x + dx, y + dy, s // 2)
                kids += j
                tus += t
        if x + s <= w and y + s <= h:
            t = tu_at(x, y, s)
            if t[3] + lam * t[4] <= kids:   # the parent wins ties
                return t[3] + lam * t[4], [(x, y, s)]
        return kids, tus

    tu = np.zeros((h // 4, w // 4), np.uint8)
    pm = np.zeros((h // 4, w // 4), np.uint8)
    lvl = np.zeros((h, w), np.int32)
    rec = np.zeros((h, w), np.int16)
    tot = np.zeros(3, np.int64)
    for cy in range(0, h, ctb):
        for cx in range(0, w, ctb):
            for x, y, n in best(cx, cy, ctb)[1]:
                l, r, m, d, rate = tu_at(x, y, n)
                lvl[y:y + n, x:x + n] = l
                rec[y:y + n, x:x + n] = r
                tu[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = int(np.log2(n))
                pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = m
                tot += (d + lam * rate, d, rate)
    return tu, pm, lvl, rec, tot


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    warnings.simplefilter("ignore")
    I, T, Q, M = _import_reference(sys.argv[1])
    out = {"numpy": np.array(np.__version__), "ncases": np.int64(len(CASES))}
    for k, (ctb, luma, (h, w), qp, lam) in enumerate(CASES):
        src = picture(h, w)
        tu, pm, lvl, rec, tot = ref_rd_plane(I, T, Q, M, src, ctb, qp, lam, luma)
        out.update({f"c{k}_src": src, f"c{k}_tu": tu, f"c{k}_pm": pm, f"c{k}_lvl": lvl, f"c{k}_rec": rec,
                    f"c{k}_stats": tot, f"c{k}_ctb": np.int64(ctb), f"c{k}_luma": np.int64(luma),
                    f"c{k}_qp": np.int64(qp), f"c{k}_lam": np.int64(lam)})
        print(f"case {k}: ctb {ctb} luma={luma} {h}x{w} qp={qp} lambda={lam}: TU sizes "
              f"{[int((tu == v).sum()) for v in range(2, 6)]} units, J/D/R {tot.tolist()}")
    np.savez_compressed(os.path.join(HERE, "tu_rd.npz"), **out)


if __name__ == "__main__":
    main()
