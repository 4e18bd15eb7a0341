"""Generate tests/golden/rdo_rd.npz by running the REFERENCE (build container only):

    python tests/golden/make_golden_rdo_rd.py REFERENCE_DIR

The 35-mode RDO with a rate term per full NxN block (DESIGN.md §3.3b open loop,
§3.7b closed loop) composed from the reference's own functions, as
make_golden_rdo.py / make_golden_rdo_closed.py compose the distortion-only
decision: BlockView neighbours (from the source plane in the open loop, from the
reconstruction Plane built so far in the closed loop), its predictors, transforms
and quantiser, ``count_nonzero`` for the rate and ``residual_energy`` for the
distortion; J = D + lam * R in Python integers, the lowest J wins, ties go to the
lowest mode.  Five kinds x two loops on the (3N+2) x (3N+3) pictures of the GPU
tests (seed 1000 + N + dst; the wide picture at N >= 16), at the QP and lambda of
tests/rdo_rd_ref.TABLE.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402
from make_golden_rdo import picture  # noqa: E402

# (n, use_dst, wide, qp, lam)
CASES = [(4, True, False, 22, 1000), (4, False, False, 22, 1000), (8, False, False, 4, 10 ** 4),
         (16, False, True, 4, 10 ** 7), (32, False, True, 4, 10 ** 7)]


def source(n, dst, wide):
    a = picture(3 * n + 2, 3 * n + 3, 1000 + n + int(dst))
    return ((a.astype(np.int32) - 128) * 32 + 128).astype(np.int16) if wide else a


def ref_plane_rd(I, T, Q, M, src, n, qp, lam, use_dst, closed):
    from nano_hevc.block import BlockView
    from nano_hevc.frame import Plane
    h, w = src.shape
    recon = Plane.zeros(h, w, np.int16)
    source_plane = Plane.zeros(h, w, np.int16)
    source_plane.data[:] = src
    modes = np.zeros((h // n, w // n), np.uint8)
    tied = np.zeros((h // n, w // n), np.uint8)
    lvl = np.zeros(src.shape, np.int32)
    sj = sd = sr = 0
    for by in range(0, h - n + 1, n):
        for bx in range(0, w - n + 1, n):
            out = BlockView(recon, bx, by, n)
            blk = out if closed else BlockView(source_plane, bx, by, n)
            orig = src[by:by + n, bx:bx + n]
            top, left, tl = blk.get_top_neighbors(), blk.get_left_neighbors(), blk.get_top_left_neighbor()
            topa = np.concatenate([[tl], blk.get_top_neighbors(2 * n)]).astype(np.int16)
            lefta = np.concatenate([[tl], blk.get_left_neighbors(n if closed else 2 * n)]).astype(np.int16)
            best, js = None, []
            for m in range(35):
                if m == 0:
                    pred = I.intra_planar_predict(top, left, int(top[-1]), int(left[-1]), n)
                elif m == 1:
                    pred = I.intra_dc_predict(top, left, n)
                else:
                    pred = I.intra_angular_predict(topa, lefta, tl, m, n)
                level = Q.quantize_block(T.forward_transform(I.residual_block(orig, pred), use_dst=use_dst), qp)
                rres = T.inverse_transform(Q.dequantize_block(level, qp), use_dst=use_dst)
                rec = I.clip_to_pixel_range(I.reconstruct_block(pred, rres.astype(np.int16)), 8)
                d = int(M.residual_energy(I.residual_block(orig, rec)))
                r = int(Q.count_nonzero(level)) + 1
                j = d + int(lam) * r
                js.append(j)
                if best is None or j < best[0]:
                    best = (j, m, level, rec, d, r)
            sj, sd, sr = sj + best[0], sd + best[4], sr + best[5]
            modes[by // n, bx // n] = best[1]
            tied[by // n, bx // n] = js.count(best[0]) > 1
            lvl[by:by + n, bx:bx + n] = best[2]
            out.write_pixels(best[3])
    return modes, lvl, np.asarray(recon.data, np.int16), np.array([sj, sd, sr], np.int64), tied


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    warnings.simplefilter("ignore")
    I, T, Q, M = _import_reference(ref)
    out = {"numpy": np.array(np.__version__), "ncases": np.int64(len(CASES))}
    for k, (n, dst, wide, qp, lam) in enumerate(CASES):
        src = source(n, dst, wide)
        out.update({f"c{k}_src": src, f"c{k}_n": np.int64(n), f"c{k}_use_dst": np.int64(dst), f"c{k}_wide": np.int64(wide),
                    f"c{k}_qp": np.int64(qp), f"c{k}_lam": np.int64(lam)})
        for loop, closed in (("open", False), ("closed", True)):
            m, l, r, st, tied = ref_plane_rd(I, T, Q, M, src, n, qp, lam, dst, closed)
            out.update({f"c{k}_{loop}_modes": m, f"c{k}_{loop}_lvl": l, f"c{k}_{loop}_rec": r, f"c{k}_{loop}_stats": st,
                        f"c{k}_{loop}_tied": tied})
            print(f"case {k} {loop}: N={n} dst={dst} qp={qp} lam={lam}: modes {m.ravel().tolist()}, "
                  f"{int(np.count_nonzero(l))} nonzero levels, stats {st.tolist()}, {int(tied.sum())} tied")
    np.savez_compressed(os.path.join(HERE, "rdo_rd.npz"), **out)


if __name__ == "__main__":
    main()
