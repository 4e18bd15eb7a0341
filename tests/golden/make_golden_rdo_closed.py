"""Generate tests/golden/rdo_closed_n.npz by running the REFERENCE (build container only):

    python tests/golden/make_golden_rdo_closed.py REFERENCE_DIR

The 35-mode CLOSED-loop RDO per full NxN block composed from the
reference's own functions, exactly as make_golden.gen_closed does for N = 8:
raster block order, neighbours fetched with BlockView from the reconstruction
Plane built so far (Plane.zeros), top reference get_top_neighbors(2N), left
reference get_left_neighbors(N), the winner written back with write_pixels.
Three 8-bit pictures and, for N = 32, a wide one: an 8-bit source quantises to
nothing at 32x32, every plane then reconstructs to 128 and every mode ties.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _chain, _import_reference  # noqa: E402
from make_golden_rdo import picture  # noqa: E402

# (n, use_dst, (h, w), qp, picture seed, wide)
CASES = [(4, True, (23, 38), 22, 101, False), (4, False, (23, 38), 30, 102, False),
         (16, False, (53, 70), 17, 103, False), (32, False, (70, 101), 4, 104, True)]


def source(h, w, seed, wide):
    a = picture(h, w, seed)
    return ((a.astype(np.int32) - 128) * 32 + 128).astype(np.int16) if wide else a


def ref_plane_rdo_closed(I, T, Q, src, n, qp, use_dst):
    from nano_hevc.block import BlockView
    from nano_hevc.frame import Plane
    h, w = src.shape
    recon = Plane.zeros(h, w, np.int16)
    modes = np.zeros((h // n, w // n), np.uint8)
    tied = np.zeros((h // n, w // n), np.uint8)
    lvl = np.zeros(src.shape, np.int32)
    total = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            blk = BlockView(recon, bx, by, n)
            orig = src[by:by + n, bx:bx + n]
            top, left, tl = blk.get_top_neighbors(), blk.get_left_neighbors(), blk.get_top_left_neighbor()
            topa = np.concatenate([[tl], blk.get_top_neighbors(2 * n)]).astype(np.int16)
            lefta = np.concatenate([[tl], blk.get_left_neighbors(n)]).astype(np.int16)
            best, costs = None, []
            for m in range(35):
                if m == 0:
                    pred = I.intra_planar_predict(top, left, int(top[-1]), int(left[-1]), n)
                elif m == 1:
                    pred = I.intra_dc_predict(top, left, n)
                else:
                    pred = I.intra_angular_predict(topa, lefta, tl, m, n)
                l, r, sse = _chain(I, T, Q, orig, pred, qp, use_dst)
                costs.append(sse)
                if best is None or sse < best[0]:
                    best = (sse, m, l, r)
            total += best[0]
            modes[by // n, bx // n] = best[1]
            tied[by // n, bx // n] = costs.count(best[0]) > 1
            lvl[by:by + n, bx:bx + n] = best[2]
            blk.write_pixels(best[3])
    return modes, lvl, np.asarray(recon.data, np.int16), total, tied


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    warnings.simplefilter("ignore")
    I, T, Q, _ = _import_reference(ref)
    out = {"numpy": np.array(np.__version__), "ncases": np.int64(len(CASES))}
    for k, (n, dst, (h, w), qp, seed, wide) in enumerate(CASES):
        src = source(h, w, seed, wide)
        m, l, r, tot, tied = ref_plane_rdo_closed(I, T, Q, src, n, qp, dst)
        out.update({f"c{k}_src": src, f"c{k}_modes": m, f"c{k}_lvl": l, f"c{k}_rec": r, f"c{k}_sse": np.int64(tot),
                    f"c{k}_tied": tied, f"c{k}_qp": np.int64(qp), f"c{k}_n": np.int64(n),
                    f"c{k}_use_dst": np.int64(dst), f"c{k}_seed": np.int64(seed), f"c{k}_wide": np.int64(wide)})
        print(f"case {k}: N={n} dst={dst} {h}x{w} qp={qp}: {len(np.unique(m))} distinct modes, "
              f"{int(np.count_nonzero(l))} nonzero levels, {len(np.unique(r))} recon values, "
              f"{int(tied.sum())} of {tied.size} blocks tied, sse {tot}")
    np.savez_compressed(os.path.join(HERE, "rdo_closed_n.npz"), **out)


if __name__ == "__main__":
    main()
