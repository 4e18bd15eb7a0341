"""CPU checks of the 35-mode RDO with a rate term: the yardstick
tests/rdo_rd_ref.py against the reference-composed records of tests/golden/rdo_rd.npz
and, at lambda = 0, against the distortion-only yardsticks; the precondition of the
GPU tests (the table's lambdas move the decisions); the 24-bit operand bounds of the
N = 8 chain; the three C ABI entry points and their host-side refusals (before any
device call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rdo_closed_ref
import rdo_rd_ref as ref
import rdo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LOOPS = [("open", False), ("closed", True)]
# blocks of 9 whose mode differs between lambda = 0 and the table's lambda (open, closed), per kind
DIFFER = {(4, True): (7, 8), (4, False): (7, 6), (8, False): (5, 7), (16, False): (7, 5), (32, False): (7, 7)}


def _walk(closed):
    return ref.rd_plane_closed if closed else ref.rd_plane


# ---- yardstick guards ----

@pytest.mark.parametrize("k", range(5))
def test_yardstick_reproduces_the_recorded_reference_cases(golden, k):
    g = golden("rdo_rd.npz")
    assert int(g["ncases"]) == 5 and str(g["numpy"]).split(".")[0] == "2"     # NEP 50 semantics (D8)
    n, dst = ref.KINDS[k]
    wide, qp, lam = ref.TABLE[(n, dst)]
    src = g[f"c{k}_src"]
    assert (int(g[f"c{k}_n"]), bool(g[f"c{k}_use_dst"]), bool(g[f"c{k}_wide"]), int(g[f"c{k}_qp"]),
            int(g[f"c{k}_lam"])) == (n, dst, wide, qp, lam)
    assert src.shape == (3 * n + 2, 3 * n + 3) and np.array_equal(src, ref.table_picture(n, dst))
    for loop, closed in LOOPS:
        m, l, r, st, tied = _walk(closed)(src, n, qp, lam, dst)
        assert np.array_equal(m, g[f"c{k}_{loop}_modes"]) and np.array_equal(l, g[f"c{k}_{loop}_lvl"]), loop
        assert np.array_equal(r, g[f"c{k}_{loop}_rec"]) and list(st) == g[f"c{k}_{loop}_stats"].tolist(), loop
        assert np.array_equal(tied, g[f"c{k}_{loop}_tied"].astype(bool)), loop
        # not degenerate: several modes, coded levels, J = D + lambda * R with a rate above the block count
        assert len(np.unique(m)) >= 3 and np.count_nonzero(l) and st[0] == st[1] + lam * st[2] and st[2] > 9
        fh, fw = 3 * n, 3 * n
        assert not r[fh:].any() and not r[:, fw:].any() and not l[fh:].any() and not l[:, fw:].any()


@pytest.mark.parametrize("n,dst", ref.KINDS)
def test_the_tables_lambda_moves_at_least_3_of_9_decisions(n, dst):
    """The precondition of the GPU tests, from the yardstick alone: a kernel that ignores lambda
    cannot pass at the table's lambda."""
    wide, qp, lam = ref.TABLE[(n, dst)]
    src = ref.table_picture(n, dst)
    counts = []
    for _, closed in LOOPS:
        m0 = _walk(closed)(src, n, qp, 0, dst)[0]
        m1 = _walk(closed)(src, n, qp, lam, dst)[0]
        assert m0.size == 9
        counts.append(int((m0 != m1).sum()))
    assert min(counts) >= 3 and tuple(counts) == DIFFER[(n, dst)]


@pytest.mark.parametrize("n,dst", ref.KINDS)
def test_lambda_0_is_the_distortion_only_decision(n, dst):
    for pic, qp in ((rdo_ref.picture, 22), (rdo_closed_ref.wide_picture, 4)):
        src = pic(2 * n + 1, 2 * n + 3, 40 + n + dst)
        m, l, r, st, _ = ref.rd_plane(src, n, qp, 0, dst)
        om, ol, orec, osse = rdo_ref.rdo_plane(src, n, qp, dst)
        assert np.array_equal(m, om) and np.array_equal(l, ol) and np.array_equal(r, orec)
        assert st[0] == st[1] == osse and st[2] == sum(
            np.count_nonzero(l[y:y + n, x:x + n]) + 1 for y in (0, n) for x in (0, n))
        m, l, r, st, tied = ref.rd_plane_closed(src, n, qp, 0, dst)
        om, ol, orec, osse = rdo_closed_ref.rdo_plane_closed(src, n, qp, dst)
        assert np.array_equal(m, om) and np.array_equal(l, ol) and np.array_equal(r, orec) and st[0] == st[1] == osse
        assert np.array_equal(tied, rdo_closed_ref.tied_blocks(src, n, qp, dst))


def test_a_plane_without_a_full_block_has_zero_stats():
    for closed in (False, True):
        for h, w in ((7, 30), (20, 7)):
            m, l, r, st, tied = _walk(closed)(rdo_ref.picture(h, w, 5), 8, 30, 1000)
            assert m.size == 0 and tuple(st) == (0, 0, 0) and not l.any() and not r.any()


def test_flat_128_costs_lambda_per_block():
    src = np.full((9, 14), 128, np.int16)
    for closed in (False, True):
        m, l, r, st, tied = _walk(closed)(src, 4, 30, 999, True)
        assert not m.any() and tuple(st) == (6 * 999, 0, 6) and tied.all() and (r[:8, :12] == 128).all()


def test_the_24_bit_operand_bounds_hold_at_8():
    """The N-lane chain at N = 8 multiplies with 24-bit operands, as at N = 4, 16 and 32: the bounds of
    tools/rdo_n_bounds.py hold for every QP (its KINDS list, which another test pins, has no N = 8)."""
    import rdo_n_bounds
    worst = 0
    for qp in range(52):
        b = rdo_n_bounds.check(8, False, qp)         # asserts every bound
        worst = max(worst, b["fwd1_operand"], b["fwd2_operand"], b["inv1_operand"], b["inv2_operand"])
    assert worst == 524288 < rdo_n_bounds.I24


# ---- C ABI ----

NAMES = ("nh_intra_rdo_rd_planes_n", "nh_intra_rdo_rd_closed_n_workspace_bytes", "nh_intra_rdo_rd_planes_closed_n")


def test_entry_points_are_exported_and_in_the_signature_table():
    from nano_hevc import _lib
    header = open(os.path.join(ROOT, "include", "nanohevc.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name in header


def _calls(L):
    from nano_hevc._lib import PlaneSet
    fake = C.c_void_p(1 << 20)   # never dereferenced: the checks return first
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)

    def sets_arg(sets):
        return sets if not isinstance(sets, PlaneSet) else C.byref(sets)

    def open_(sets=ok, nsets=1, n=16, dst=0, qp=30, lam=100, ptrs=None):
        p = ptrs or [fake] * 5   # src, modes, lvl, recon, stats
        return L.nh_intra_rdo_rd_planes_n(p[0], sets_arg(sets) if sets is not None else None, nsets, n, dst, qp, lam,
                                          p[1], p[2], p[3], p[4], None)

    def closed(sets=ok, nsets=1, n=16, dst=0, qp=30, lam=100, ptrs=None):
        p = ptrs or [fake] * 6   # src, modes, lvl, recon, stats, work
        return L.nh_intra_rdo_rd_planes_closed_n(p[0], sets_arg(sets) if sets is not None else None, nsets, n, dst, qp,
                                                 lam, p[1], p[2], p[3], p[4], p[5], None)

    return [(open_, 5, b"nh_intra_rdo_rd_planes_n"), (closed, 6, b"nh_intra_rdo_rd_planes_closed_n")]


@pytest.mark.parametrize("which", [0, 1])
def test_refusals_precede_any_device_call(which):
    """Every refusal returns NH_EARG on the host with the entry point's name and the offending word in
    nh_last_error; the pointers are fakes that no device call could survive."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    call, nptr, name = _calls(L)[which]
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    sets9 = (PlaneSet * 9)(*([ok] * 9))

    def refused(rc, text):
        assert rc == _lib.NH_EARG
        err = L.nh_last_error()
        assert name in err and text in err, err

    for n in (0, 2, 5, 12, 64, -4):
        refused(call(n=n), b"block_size")
    for n in (8, 16, 32):
        refused(call(n=n, dst=1), b"use_dst")
    for n in (4, 8, 16, 32):
        for qp in (-1, 52, 1000):
            refused(call(n=n, qp=qp), b"qp")
        for lam in (-1, 1 << 31, 1 << 40):
            refused(call(n=n, lam=lam), b"lambda")
        for nsets in (0, -1, 9):
            refused(call(sets=sets9, nsets=nsets, n=n), b"nsets")
    bad = [PlaneSet(0, 0, 0, 64, 64, 63, 1, 1, 0),      # pitch < width
           PlaneSet(-8, 0, 0, 64, 64, 64, 1, 1, 0),     # negative base
           PlaneSet(0, -1, 0, 64, 64, 64, 2, 1, 0),     # negative plane stride
           PlaneSet(0, 0, 0, 64, 64, 64, 0, 1, 0),      # no plane per group
           PlaneSet(0, 0, 0, -1, 64, 64, 1, 1, 0),      # negative width
           PlaneSet(0, 0, 0, 64, 64, 64, 256, 256, 0)]  # more than 65535 planes
    if which == 1:
        bad.append(PlaneSet(0, 0, 0, 70000, 64, 70000, 1, 1, 0))   # wider than the line words address
    for s in bad:
        for n in (4, 8, 16, 32):
            refused(call(sets=s, n=n), b"plane set")
    fake = C.c_void_p(1 << 20)
    for i in range(nptr):
        ptrs = [fake] * nptr
        ptrs[i] = None
        refused(call(ptrs=ptrs), b"null")
    refused(call(sets=None), b"null")
    ptrs = [fake] * nptr
    ptrs[4] = None                     # the null stats pointer is refused before the QP
    for n in (4, 8, 16, 32):
        refused(call(n=n, qp=52, ptrs=ptrs), b"null")
    odd = [fake] * nptr
    odd[4] = C.c_void_p((1 << 20) + 4)
    refused(call(ptrs=odd), b"d_stats")
    if which == 1:
        odd = [fake] * nptr
        odd[5] = C.c_void_p((1 << 20) + 4)
        refused(call(ptrs=odd), b"workspace")


def test_sets_without_a_plane_launch_nothing():
    """The open form returns 0 without touching the device (there is no stats word to zero) at the limits
    of QP and lambda; planes without a full block are zeroed on the device (test_rdo_rd_gpu.py)."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    open_ = _calls(L)[0][0]
    for s in (PlaneSet(0, 0, 0, 64, 64, 64, 1, 0, 0), PlaneSet(0, 0, 0, 3, 3, 3, 2, 0, 0)):
        for qp, lam in ((0, 0), (51, (1 << 31) - 1)):
            for n, dst in ref.KINDS:
                assert open_(sets=s, n=n, dst=int(dst), qp=qp, lam=lam) == _lib.NH_OK


def test_workspace_size():
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    size = L.nh_intra_rdo_rd_closed_n_workspace_bytes
    sets = (PlaneSet * 2)(PlaneSet(0, 0, 0, 70, 53, 70, 1, 3, 53 * 70), PlaneSet(3 * 53 * 70, 24 * 40, 0, 40, 24, 40, 2, 1, 0))
    for n in (4, 8, 16, 32):
        # per plane (w + 1) / 2 + N line words of 8 bytes, after the ticket and the status word: at N = 8 too
        assert size(sets, 2, n) == 8 + 8 * (3 * (35 + n) + 2 * (20 + n)), n
    assert size(sets, 2, 8) != L.nh_intra_rdo_closed_workspace_bytes(sets, 2) > 0   # N = 8 is not forwarded
    assert size(None, 1, 16) < 0 and b"null" in L.nh_last_error()
    for n in (0, 12, 64):
        assert size(sets, 2, n) < 0 and b"block_size" in L.nh_last_error(), n
    for nsets in (0, 9):
        assert size(sets, nsets, 16) < 0 and b"nsets" in L.nh_last_error(), nsets
    for n in (4, 8, 16, 32):
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 63, 1, 1, 0)), 1, n) < 0, n      # pitch < width
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 64, 0, 1, 0)), 1, n) < 0, n      # no plane per group
        assert size(C.byref(PlaneSet(0, 0, 0, 70000, 64, 70000, 1, 1, 0)), 1, n) < 0, n   # wider than 65535
        assert b"plane set" in L.nh_last_error()
