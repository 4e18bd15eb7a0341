"""Generate tests/golden/rdo_n.npz by running the REFERENCE (build container only):

    python tests/golden/make_golden_rdo.py REFERENCE_DIR

The 35-mode open-loop RDO per full NxN block composed from the
reference's own functions, exactly as make_golden.ref_plane_cfg3 does for N = 8,
for four 8-bit pictures (full-range int16 planes make the reference's planar
store raise, D9; those are compared with the oracle yardstick alone).
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _chain, _import_reference, _neighbors  # noqa: E402

# (n, use_dst, (h, w), qp, picture seed)
CASES = [(4, True, (23, 38), 22, 101), (4, False, (23, 38), 30, 102),
         (16, False, (53, 70), 17, 103), (32, False, (70, 101), 4, 104)]


def picture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = (128 + 60 * np.sin(x / 5 + y / 9) + 40 * np.cos(y / 3 - x / 11) + rng.integers(-6, 7, (h, w))).clip(0, 255)
    a[h // 2:, w // 3:] = (a[h // 2:, w // 3:] // 32) * 32
    return a.astype(np.int16)


def ref_plane_rdo(I, T, Q, src, n, qp, use_dst):
    h, w = src.shape
    modes = np.zeros((h // n, w // n), np.uint8)
    lvl = np.zeros(src.shape, np.int32)
    rec = np.zeros(src.shape, np.int16)
    total = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            orig = src[by:by + n, bx:bx + n]
            top, left, tl = _neighbors(src, bx, by, n)
            top2, left2, _ = _neighbors(src, bx, by, 2 * n)
            topa = np.concatenate([[tl], top2]).astype(np.int16)
            lefta = np.concatenate([[tl], left2]).astype(np.int16)
            best = None
            for m in range(35):
                if m == 0:
                    pred = I.intra_planar_predict(top, left, int(top[-1]), int(left[-1]), n)
                elif m == 1:
                    pred = I.intra_dc_predict(top, left, n)
                else:
                    pred = I.intra_angular_predict(topa, lefta, tl, m, n)
                l, r, sse = _chain(I, T, Q, orig, pred, qp, use_dst)
                if best is None or sse < best[0]:
                    best = (sse, m, l, r)
            total += best[0]
            modes[by // n, bx // n] = best[1]
            lvl[by:by + n, bx:bx + n] = best[2]
            rec[by:by + n, bx:bx + n] = best[3]
    return modes, lvl, rec, total


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    warnings.simplefilter("ignore")
    I, T, Q, _ = _import_reference(ref)
    out = {"numpy": np.array(np.__version__), "ncases": np.int64(len(CASES))}
    for k, (n, dst, (h, w), qp, seed) in enumerate(CASES):
        src = picture(h, w, seed)
        m, l, r, tot = ref_plane_rdo(I, T, Q, src, n, qp, dst)
        out.update({f"c{k}_src": src, f"c{k}_modes": m, f"c{k}_lvl": l, f"c{k}_rec": r, f"c{k}_sse": np.int64(tot),
                    f"c{k}_qp": np.int64(qp), f"c{k}_n": np.int64(n), f"c{k}_use_dst": np.int64(dst),
                    f"c{k}_seed": np.int64(seed)})
        print(f"case {k}: N={n} dst={dst} {h}x{w} qp={qp}: {len(np.unique(m))} distinct modes, "
              f"{int(np.count_nonzero(l))} nonzero levels, sse {tot}")
    np.savez_compressed(os.path.join(HERE, "rdo_n.npz"), **out)


if __name__ == "__main__":
    main()
