"""Test helper: the closed-loop intra decoder at block size N
restated on the CPU from the pinned oracle's primitives only -- what
``gpu.dequant_inv_n`` and ``gpu.intra_decode_closed_n`` are compared with.  It is
``decode_ref.decode`` with ``use_dst`` passed to ``O.inverse_transform``: at N = 8
the two are equal, and it reproduces the reference-composed reconstructions of
tests/golden/rdo_closed_n.npz from their modes and levels bit-exactly
(test_decode_n_host.py).  Also the two input families that the host and the GPU
tests share: every mode at every position class, and the int16 wrap."""
import functools

import numpy as np

from oracle import oracle as O

KINDS = ((4, True), (4, False), (16, False), (32, False))     # (N, use_dst)


def residual_block(level, qp, use_dst=False):
    """Stage R of one block: inverse_transform(dequantize_block(level, qp), use_dst).astype(int16)."""
    return O.inverse_transform(O.dequantize(level, qp), use_dst).astype(np.int16)


def residual_plane(lvl, qp, out, N, use_dst=False):
    """Stage R over the full blocks of one plane, written into ``out`` (rest untouched)."""
    h, w = lvl.shape
    for by in range(0, h - N + 1, N):
        for bx in range(0, w - N + 1, N):
            out[by:by + N, bx:bx + N] = residual_block(lvl[by:by + N, bx:bx + N], qp, use_dst)
    return out


def decode(modes, lvl, qp, N, use_dst=False, reconstruct=None):
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
            r = residual_block(lvl[by:by + N, bx:bx + N], qp, use_dst)
            rec[by:by + N, bx:bx + N] = reconstruct(pred, r) if reconstruct else O.clip(O.reconstruct(pred, r), 8)
    return rec


def saturating_reconstruct(pred, res):
    """The variant the wrap inputs tell from the reference: the add in more than 16 bits, then the clip."""
    return np.clip(pred.astype(np.int32) + res.astype(np.int32), 0, 255).astype(np.int16)


# ------------------------------------------------------------------ every mode at every position class

# (N, use_dst) -> (amplitude, density, QP) of the sparse random int32 levels.  N = 32: of the two inputs
# found on the CPU, (+-120, 0.01, QP 27) and (+-1500, 0.02, QP 4), the first.
EVERY_MODE = {(4, True): (3, 0.5, 22), (4, False): (3, 0.5, 22), (16, False): (12, 0.08, 27), (32, False): (120, 0.01, 27)}
EVERY_MODE_PLANES = 35
RAILED_CAP = 0.15


def every_mode_shape(n):
    return 3 * n + 2, 3 * n + 3


@functools.lru_cache(maxsize=None)
def every_mode(n, dst):
    """(modes (35, 3, 3) uint8, lvl (35, h, w) int32, qp, rec (35, h, w) int16 of ``decode``), read only:
    block (i, j) of plane p has mode (p + 3 i + j) mod 35, so every mode sits at the corner, in the first
    row, the first column, the interior and the last column (top-right reference truncated at the plane's
    edge, 0 past the last full block)."""
    amp, dens, qp = EVERY_MODE[(n, dst)]
    h, w = every_mode_shape(n)
    rng = np.random.default_rng(9000 + n + dst)
    p, i, j = np.mgrid[0:EVERY_MODE_PLANES, 0:3, 0:3]
    modes = ((p + 3 * i + j) % 35).astype(np.uint8)
    lvl = (rng.integers(-amp, amp + 1, (EVERY_MODE_PLANES, h, w)) *
           (rng.random((EVERY_MODE_PLANES, h, w)) < dens)).astype(np.int32)
    rec = np.stack([decode(modes[k], lvl[k], qp, n, dst) for k in range(EVERY_MODE_PLANES)])
    for a in (modes, lvl, rec):
        a.setflags(write=False)
    return modes, lvl, qp, rec


def every_mode_census(n, dst):
    """(blocks, blocks with a nonzero residual, blocks whose recon is constant, share of the full-block
    samples at 0 or 255) of the helper's own output on the ``every_mode`` input."""
    _, lvl, qp, rec = every_mode(n, dst)
    blocks = nonzero = constant = 0
    for k in range(EVERY_MODE_PLANES):
        res = residual_plane(lvl[k], qp, np.zeros(lvl[k].shape, np.int16), n, dst)
        for by in range(0, 3 * n, n):
            for bx in range(0, 3 * n, n):
                blocks += 1
                nonzero += bool(res[by:by + n, bx:bx + n].any())
                constant += len(np.unique(rec[k, by:by + n, bx:bx + n])) == 1
    inside = rec[:, :3 * n, :3 * n]
    return blocks, nonzero, constant, float(((inside == 0) | (inside == 255)).mean())


# ------------------------------------------------------------------ the int16 wrap

# (N, use_dst) -> (L, QP, largest residual, samples in which the saturating variant differs)
WRAP = {(4, False): (160, 50, 32640, 16), (16, False): (2291, 51, 32647, 256), (32, False): (9162, 51, 32640, 1024),
        (4, True): (93, 50, 32683, 1)}


def wrap_input(n, dst):
    """(modes, lvl, qp) of a 2N x 2N plane, every mode 1: level 1 at (0, 0), level L at (N, N), whose
    residual exceeds 32767 - 128 -- the int16 add of prediction and residual wraps below zero."""
    L, qp, _, _ = WRAP[(n, dst)]
    lvl = np.zeros((2 * n, 2 * n), np.int32)
    lvl[0, 0] = 1
    lvl[n, n] = L
    return np.ones((2, 2), np.uint8), lvl, qp
