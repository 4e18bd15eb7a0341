"""Test helper: the config-4 closed-loop decoder restated on the
CPU from the pinned oracle's primitives only -- what ``gpu.tu_pred_map_closed``,
``gpu.dequant_inv_tu`` and ``gpu.tu_decode_closed`` are compared with.  ``decode``
on the map ``pred_map`` derives reproduces the reference's own recorded config-4
closed-loop reconstructions (tests/golden/closed4.npz): test_tu_decode_host.py."""
import numpy as np

from oracle import oracle as O


def valid(tu, ctb):
    """Map validity: every unit value v in [2, log2 ctb], the aligned n x n square
    (n = 1 << v) holding the unit inside the plane, every unit of that square v."""
    tu = np.asarray(tu)
    h4, w4 = tu.shape
    top = {4: 2, 8: 3, 16: 4, 32: 5}[ctb]
    for uy in range(h4):
        for ux in range(w4):
            v = int(tu[uy, ux])
            if v < 2 or v > top:
                return False
            nu = 1 << (v - 2)
            ox, oy = ux - ux % nu, uy - uy % nu
            if ox + nu > w4 or oy + nu > h4 or not (tu[oy:oy + nu, ox:ox + nu] == v).all():
                return False
    return True


def tus(tu, ctb):
    """(x, y, N) of every TU of a valid map: CTUs in raster order, z-order inside a CTU."""
    tu = np.asarray(tu)
    h4, w4 = tu.shape
    out = []

    def walk(x, y, s):
        if x >= 4 * w4 or y >= 4 * h4:
            return
        if int(tu[y // 4, x // 4]) == int(np.log2(s)):
            out.append((x, y, s))
            return
        assert s > 4, "not a valid map"
        for dy in (0, s // 2):
            for dx in (0, s // 2):
                walk(x + dx, y + dy, s // 2)

    for cy in range(0, 4 * h4, ctb):
        for cx in range(0, 4 * w4, ctb):
            walk(cx, cy, ctb)
    assert sum(n * n for _, _, n in out) == 16 * h4 * w4
    return out


def _neighbours(rec, x, y, n):
    """BlockView.get_top / get_left_neighbors: n samples, 128 at the plane border."""
    top = np.full(n, 128, np.int16) if y == 0 else rec[y - 1, x:x + n].copy()
    left = np.full(n, 128, np.int16) if x == 0 else rec[y:y + n, x - 1].copy()
    return top, left


def _preds(rec, x, y, n):
    top, left = _neighbours(rec, x, y, n)
    return O.intra_dc(top, left, n), O.intra_planar(top, left, top[-1], left[-1], n)


def pred_energies(src, rec, x, y, n):
    """(e_dc, e_planar) of the TU (x, y, n): int16-wrapping residual, int64 energies."""
    o = src[y:y + n, x:x + n]
    return tuple(int((O.residual(o, p).astype(np.int64) ** 2).sum()) for p in _preds(rec, x, y, n))


def pred_map(src, rec, tu, ctb):
    """1 = DC where e_dc <= e_planar (int16-wrapping residual, int64 energies), else 0;
    written to every unit of the TU."""
    pm = np.zeros_like(np.asarray(tu, np.uint8))
    for x, y, n in tus(tu, ctb):
        e = pred_energies(src, rec, x, y, n)
        pm[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = 1 if e[0] <= e[1] else 0
    return pm


def residual_tu(level, qp, use_dst):
    """Stage R of one TU."""
    return O.inverse_transform(O.dequantize(level, qp), use_dst).astype(np.int16)


def residual(lvl, tu, ctb, qp, is_luma, out=None):
    """Stage R over the TUs of one plane, written into ``out``."""
    out = np.zeros(lvl.shape, np.int16) if out is None else out
    for x, y, n in tus(tu, ctb):
        out[y:y + n, x:x + n] = residual_tu(lvl[y:y + n, x:x + n], qp, bool(is_luma) and n == 4)
    return out


def decode(tu, pm, lvl, ctb, qp, is_luma, reconstruct=None):
    """``reconstruct(pred, res) -> samples`` replaces the reference's wrapping int16 add and clip:
    only for tests that show their inputs tell the reference from a variant of it."""
    rec = np.zeros(lvl.shape, np.int16)
    for x, y, n in tus(tu, ctb):
        dc, pl = _preds(rec, x, y, n)
        m = int(pm[y // 4, x // 4])
        assert m in (0, 1)
        pred = dc if m == 1 else pl
        r = residual_tu(lvl[y:y + n, x:x + n], qp, bool(is_luma) and n == 4)
        rec[y:y + n, x:x + n] = reconstruct(pred, r) if reconstruct else O.clip(O.reconstruct(pred, r), 8)
    return rec
