"""CPU checks of the NxN 35-mode RDO: the yardstick
tests/rdo_ref.py against the oracle's own 8x8 driver and against the
reference-composed records of tests/golden/rdo_n.npz; the C ABI entry point, its
host-side refusals (before any device call), and the operand bounds of the
kernel's 24-bit multiplies (tools/rdo_n_bounds.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rdo_ref
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


# ---- yardstick guards ----

def test_rdo_ref_equals_the_oracle_driver_at_8():
    src = rdo_ref.picture(43, 61, 7)
    m, l, r, s = rdo_ref.rdo_plane(src, 8, 27)
    om, ol, orec, osse = O.intra_rdo_plane(src, 27)
    assert np.array_equal(m, om) and np.array_equal(l, ol) and np.array_equal(r, orec) and s == osse
    assert len(np.unique(m)) >= 3 and np.count_nonzero(l)


@pytest.mark.parametrize("k", range(4))
def test_rdo_ref_reproduces_the_recorded_reference_cases(golden, k):
    g = golden("rdo_n.npz")
    assert int(g["ncases"]) == 4 and str(g["numpy"]).split(".")[0] == "2"     # NEP 50 semantics (D8)
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    src = g[f"c{k}_src"]
    assert (n, dst, src.shape, qp) == [(4, True, (23, 38), 22), (4, False, (23, 38), 30), (16, False, (53, 70), 17),
                                      (32, False, (70, 101), 4)][k]
    assert np.array_equal(src, rdo_ref.picture(*src.shape, int(g[f"c{k}_seed"])))
    m, l, r, s = rdo_ref.rdo_plane(src, n, qp, dst)
    assert np.array_equal(m, g[f"c{k}_modes"]) and np.array_equal(l, g[f"c{k}_lvl"])
    assert np.array_equal(r, g[f"c{k}_rec"]) and s == int(g[f"c{k}_sse"])
    assert np.count_nonzero(l) and rdo_ref.has_tie(src, n, qp, dst)


# ---- C ABI ----

def test_entry_point_is_exported_and_in_the_signature_table():
    from nano_hevc import _lib
    assert "nh_intra_rdo_planes_n" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "nh_intra_rdo_planes_n")
    assert "nh_intra_rdo_planes_n" in open(os.path.join(ROOT, "include", "nanohevc.h")).read()


def test_refusals_precede_any_device_call():
    """Every refusal returns NH_EARG on the host with its text in nh_last_error; the
    pointers are fakes that no device call could survive."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    fake = C.c_void_p(1 << 20)
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    sets8 = (PlaneSet * 9)(*([ok] * 9))

    def call(sets=ok, nsets=1, n=16, dst=0, qp=30):
        arr = sets if not isinstance(sets, PlaneSet) else C.byref(sets)
        return L.nh_intra_rdo_planes_n(fake, arr, nsets, n, dst, qp, fake, fake, fake, fake, None)

    for n in (0, 2, 5, 12, 64, -4):
        assert call(n=n) == _lib.NH_EARG, n
        assert b"block_size" in L.nh_last_error()
    for n in (8, 16, 32):
        assert call(n=n, dst=1) == _lib.NH_EARG, n
        assert b"use_dst" in L.nh_last_error()
    for n in (4, 8, 16, 32):               # block_size 8 is checked before it is forwarded
        for qp in (-1, 52, 1000):
            assert call(n=n, qp=qp) == _lib.NH_EARG, (n, qp)
            assert b"qp" in L.nh_last_error()
        for nsets in (0, -1, 9):
            assert call(sets=sets8, nsets=nsets, n=n) == _lib.NH_EARG, (n, nsets)
            assert b"nsets" in L.nh_last_error()
    bad = [PlaneSet(0, 0, 0, 64, 64, 63, 1, 1, 0),      # pitch < width
           PlaneSet(-8, 0, 0, 64, 64, 64, 1, 1, 0),     # negative base
           PlaneSet(0, -1, 0, 64, 64, 64, 2, 1, 0),     # negative plane stride
           PlaneSet(0, 0, 0, 64, 64, 64, 0, 1, 0),      # no plane per group
           PlaneSet(0, 0, 0, -1, 64, 64, 1, 1, 0),      # negative width
           PlaneSet(0, 0, 0, 64, 64, 64, 256, 256, 0)]  # more than 65535 planes
    for s in bad:
        assert call(sets=s, n=4) == _lib.NH_EARG
        assert b"plane set" in L.nh_last_error()
    assert L.nh_intra_rdo_planes_n(None, C.byref(ok), 1, 16, 0, 30, fake, fake, fake, fake, None) == _lib.NH_EARG


def test_the_sse_pointer_is_optional_in_the_open_loop_only():
    """nh_intra_rdo_planes_n takes d_sse = NULL: with QP 52 besides, the refusal is the QP's.  The closed
    loop needs its sums: the same call on nh_intra_rdo_planes_closed_n is refused for the null pointer,
    which comes first."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    fake = C.c_void_p(1 << 20)
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    for n in (4, 8, 16, 32):
        assert L.nh_intra_rdo_planes_n(fake, C.byref(ok), 1, n, 0, 52, fake, fake, fake, None, None) == _lib.NH_EARG, n
        err = L.nh_last_error()
        assert b"nh_intra_rdo_planes_n:" in err and b"qp" in err and b"null" not in err, err
        assert L.nh_intra_rdo_planes_closed_n(fake, C.byref(ok), 1, n, 0, 52, fake, fake, fake, None, fake,
                                              None) == _lib.NH_EARG, n
        err = L.nh_last_error()
        assert b"nh_intra_rdo_planes_closed_n:" in err and b"null" in err, err


def test_sets_without_a_full_block_launch_nothing():
    """A set smaller than N in one dimension (or without planes) holds no block: the call
    returns NH_OK without touching the device (fake pointers again)."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    fake = C.c_void_p(1 << 20)
    for n in (4, 16, 32):
        sets = (PlaneSet * 3)(PlaneSet(0, 0, 0, n - 1, 5 * n, 5 * n, 1, 2, 0), PlaneSet(0, 0, 0, 3 * n, n - 1, 3 * n, 2, 1, 0),
                              PlaneSet(0, 0, 0, 2 * n, 2 * n, 2 * n, 1, 0, 0))
        assert L.nh_intra_rdo_planes_n(fake, sets, 3, n, 0, 30, fake, fake, fake, fake, None) == _lib.NH_OK, n


# ---- the 24-bit multiplies ----

def test_mul24_operand_bounds_for_every_qp_and_transform():
    import rdo_n_bounds as rb
    assert rb.KINDS == ((4, True), (4, False), (16, False), (32, False))
    worst = 0
    for n, dst in rb.KINDS:
        for qp in range(52):
            b = rb.check(n, dst, qp)        # asserts each bound
            worst = max(worst, b["fwd1_operand"], b["fwd2_operand"], b["inv1_operand"], b["inv2_operand"], b["level"])
            assert b["coef"] <= 1 << 17
    assert worst == 2097152 < 1 << 23       # DCT32's second forward pass: 32 * 2^16


def test_mul24_bounds_checker_catches_a_wider_residual():
    """The enumeration is not vacuous: a 20-bit residual breaks DCT32's forward operands."""
    import rdo_n_bounds as rb
    b = rb.bounds(32, False, 0, x0=1 << 20)
    assert b["fwd2_operand"] >= 1 << 23 and b["coef"] > 1 << 17
