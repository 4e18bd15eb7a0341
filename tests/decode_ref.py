"""Test helper: the closed-loop intra decoder restated on the
CPU from the pinned oracle's primitives only -- what ``gpu.intra_decode_closed``
is compared with.  ``decode`` reproduces the reference's own recorded closed-loop
reconstructions (tests/golden/closed.npz) bit-exactly: test_decode_host.py."""
import numpy as np

from oracle import oracle as O


def residual_block(level, qp):
    """Stage R of one block: inverse_transform(dequantize_block(level, qp)).astype(int16)."""
    return O.inverse_transform(O.dequantize(level, qp)).astype(np.int16)


def residual_plane(lvl, qp, out, N=8):
    """Stage R over the full blocks of one plane, written into ``out`` (rest untouched)."""
    h, w = lvl.shape
    for by in range(0, h - N + 1, N):
        for bx in range(0, w - N + 1, N):
            out[by:by + N, bx:bx + N] = residual_block(lvl[by:by + N, bx:bx + N], qp)
    return out


def decode(modes, lvl, qp, N=8, reconstruct=None):
    """``reconstruct(pred, res) -> samples`` replaces the reference's wrapping int16 add and clip:
    only for tests that show their inputs tell the reference from a variant of it."""
    h, w = lvl.shape
    rec = np.zeros((h, w), np.int16)
    for by in range(0, h - N + 1, N):
        for bx in range(0, w - N + 1, N):
            m = int(modes[by // N, bx // N])
            top = lambda n: np.full(n, 128, np.int16) if by == 0 else rec[by - 1, bx:bx + n].copy()
            left = np.full(N, 128, np.int16) if bx == 0 else rec[by:by + N, bx - 1].copy()
            tl = 128 if (bx == 0 or by == 0) else int(rec[by - 1, bx - 1])
            if m == 0:
                t = top(N); pred = O.intra_planar(t, left, t[-1], left[-1], N)
            elif m == 1:
                pred = O.intra_dc(top(N), left, N)
            else:
                pred = O.intra_angular(np.concatenate([[tl], top(2 * N)]), np.concatenate([[tl], left]), tl, m, N)
            r = O.inverse_transform(O.dequantize(lvl[by:by + N, bx:bx + N], qp)).astype(np.int16)
            rec[by:by + N, bx:bx + N] = reconstruct(pred, r) if reconstruct else O.clip(O.reconstruct(pred, r), 8)
    return rec
