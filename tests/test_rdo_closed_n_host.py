"""CPU checks of the NxN 35-mode CLOSED-loop RDO: the yardstick
tests/rdo_closed_ref.py against the oracle's own closed 8x8 driver and against the
reference-composed records of tests/golden/rdo_closed_n.npz; the 8-bit degeneracy
at N = 32 that the wide fixture exists for; the two C ABI entry points and their
host-side refusals (before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest

import rdo_closed_ref as ref
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, use_dst, shape, qp, seed, wide, distinct chosen modes, tied blocks, blocks)
CASES = [(4, True, (23, 38), 22, 101, False, 28, 2, 45), (4, False, (23, 38), 30, 102, False, 18, 1, 45),
         (16, False, (53, 70), 17, 103, False, 10, 1, 12), (32, False, (70, 101), 4, 104, True, 4, 1, 6)]


# ---- yardstick guards ----

def test_yardstick_equals_the_oracle_closed_driver_at_8():
    src = ref.picture(43, 61, 7)
    m, l, r, s = ref.rdo_plane_closed(src, 8, 27)
    om, ol, orec, osse = O.intra_rdo_plane(src, 27, closed=True)
    assert np.array_equal(m, om) and np.array_equal(l, ol) and np.array_equal(r, orec) and s == osse
    assert len(np.unique(m)) >= 3 and np.count_nonzero(l)


@pytest.mark.parametrize("k", range(4))
def test_recorded_cases_are_what_the_issue_lists_and_not_degenerate(golden, k):
    g = golden("rdo_closed_n.npz")
    assert int(g["ncases"]) == 4 and str(g["numpy"]).split(".")[0] == "2"     # NEP 50 semantics (D8)
    n, dst, shape, qp, seed, wide, nmodes, ntied, nblk = CASES[k]
    src = g[f"c{k}_src"]
    assert (int(g[f"c{k}_n"]), bool(g[f"c{k}_use_dst"]), src.shape, int(g[f"c{k}_qp"]), int(g[f"c{k}_seed"]),
            bool(g[f"c{k}_wide"])) == (n, dst, shape, qp, seed, wide)
    assert np.array_equal(src, ref.wide_picture(*shape, seed) if wide else ref.picture(*shape, seed))
    if wide:
        assert src.min() < -3000 and src.max() > 3000
    modes, lvl, rec, tied = g[f"c{k}_modes"], g[f"c{k}_lvl"], g[f"c{k}_rec"], g[f"c{k}_tied"]
    assert len(np.unique(modes)) >= 3 and np.count_nonzero(lvl) and len(np.unique(rec)) > 2
    assert tied.any() and not tied.all()
    assert (len(np.unique(modes)), int(tied.sum()), tied.size) == (nmodes, ntied, nblk)
    fh, fw = shape[0] // n * n, shape[1] // n * n
    assert not rec[fh:].any() and not rec[:, fw:].any() and not lvl[fh:].any() and not lvl[:, fw:].any()


@pytest.mark.parametrize("k", range(4))
def test_yardstick_reproduces_the_recorded_reference_cases(golden, k):
    g = golden("rdo_closed_n.npz")
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    src = g[f"c{k}_src"]
    m, l, r, s = ref.rdo_plane_closed(src, n, qp, dst)
    assert np.array_equal(m, g[f"c{k}_modes"]) and np.array_equal(l, g[f"c{k}_lvl"])
    assert np.array_equal(r, g[f"c{k}_rec"]) and s == int(g[f"c{k}_sse"])
    assert np.array_equal(ref.tied_blocks(src, n, qp, dst), g[f"c{k}_tied"].astype(bool))
    assert ref.has_tie(src, n, qp, dst)


def test_an_8_bit_source_degenerates_at_32():
    """Why the N = 32 fixture is wide: 8-bit coefficients are at most about 100 under the same-shift
    scaling, every reconstructed residual is 0 (whatever the levels), the recon is the prediction --
    128 from the border on."""
    src = ref.picture(70, 101, 104)
    m, l, r, s = ref.rdo_plane_closed(src, 32, 4)
    assert not m.any()
    assert (r[:64, :96] == 128).all() and not r[64:].any() and not r[:, 96:].any()
    assert ref.tied_blocks(src, 32, 4).all() and not ref.has_tie(src, 32, 4)
    assert s == int(((src[:64, :96].astype(np.int64) - 128) ** 2).sum())


# ---- C ABI ----

NAMES = ("nh_intra_rdo_closed_n_workspace_bytes", "nh_intra_rdo_planes_closed_n")


def test_entry_points_are_exported_and_in_the_signature_table():
    from nano_hevc import _lib
    header = open(os.path.join(ROOT, "include", "nanohevc.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name in header


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
        return L.nh_intra_rdo_planes_closed_n(fake, arr, nsets, n, dst, qp, fake, fake, fake, fake, fake, None)

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
        for n in (4, 8, 16, 32):
            assert call(sets=s, n=n) == _lib.NH_EARG, n
            assert b"plane set" in L.nh_last_error()
    for null in range(7):                  # src, sets, modes, lvl, recon, sse, work
        args = [fake, C.byref(ok), 1, 16, 0, 30, fake, fake, fake, fake, fake, None]
        args[(0, 1, 6, 7, 8, 9, 10)[null]] = None
        assert L.nh_intra_rdo_planes_closed_n(*args) == _lib.NH_EARG, null
        assert b"null" in L.nh_last_error()


def test_workspace_size():
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    size = L.nh_intra_rdo_closed_n_workspace_bytes
    sets = (PlaneSet * 2)(PlaneSet(0, 0, 0, 70, 53, 70, 1, 3, 53 * 70), PlaneSet(3 * 53 * 70, 24 * 40, 0, 40, 24, 40, 2, 1, 0))
    for n in (4, 16, 32):
        # per plane (w + 1) / 2 + N line words of 8 bytes, after the ticket and the status word
        assert size(sets, 2, n) == 8 + 8 * (3 * (35 + n) + 2 * (20 + n)), n
    assert size(sets, 2, 8) == L.nh_intra_rdo_closed_workspace_bytes(sets, 2) > 0
    assert size(None, 1, 16) < 0
    for n in (0, 12, 64):
        assert size(sets, 2, n) < 0, n
    for nsets in (0, 9):
        assert size(sets, nsets, 16) < 0, nsets
    for n in (4, 8, 16, 32):
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 63, 1, 1, 0)), 1, n) < 0, n      # pitch < width
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 64, 0, 1, 0)), 1, n) < 0, n      # no plane per group
    assert size(C.byref(PlaneSet(0, 0, 0, 70000, 64, 70000, 1, 1, 0)), 1, 16) < 0       # wider than 65535
