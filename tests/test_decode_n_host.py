"""CPU checks of the closed-loop decoder at N = 4, 16, 32: the
helper tests/decode_n_ref.py against the reference-composed records of
tests/golden/rdo_closed_n.npz, against ``decode_ref.decode`` at N = 8 and against
the encoder yardstick tests/rdo_closed_ref.py; the shared input families of the GPU
tests (every mode, int16 wrap) against their caps; the three C ABI entry points
and their host-side refusals (before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest

import decode_n_ref as dn
import decode_ref
import rdo_closed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the recorded reference cases ----

@pytest.mark.parametrize("k", range(4))
def test_helper_reproduces_the_recorded_reconstructions(golden, k):
    g = golden("rdo_closed_n.npz")
    n, qp, dst = int(g[f"c{k}_n"]), int(g[f"c{k}_qp"]), bool(g[f"c{k}_use_dst"])
    got = dn.decode(g[f"c{k}_modes"], g[f"c{k}_lvl"], qp, n, dst)
    assert np.array_equal(got, g[f"c{k}_rec"])
    if n == 4:   # the fixtures tell the two 4x4 transforms apart
        assert not np.array_equal(dn.decode(g[f"c{k}_modes"], g[f"c{k}_lvl"], qp, n, not dst), g[f"c{k}_rec"])


# ---- 2. N = 8 ----

def test_helper_equals_decode_ref_at_8():
    rng = np.random.default_rng(21)
    modes = rng.integers(0, 35, (4, 5)).astype(np.uint8)
    lvl = rng.integers(-3, 4, (37, 43)).astype(np.int32)
    want = decode_ref.decode(modes, lvl, 27)
    assert np.array_equal(dn.decode(modes, lvl, 27, 8), want) and len(np.unique(want)) > 50
    out_a, out_b = np.full(lvl.shape, -7, np.int16), np.full(lvl.shape, -7, np.int16)
    assert np.array_equal(dn.residual_plane(lvl, 27, out_a, 8), decode_ref.residual_plane(lvl, 27, out_b))


# ---- 3. the encoder yardstick ----

@pytest.mark.parametrize("n,dst", dn.KINDS)
def test_helper_equals_the_encoder_yardstick(n, dst):
    src = ref.wide_picture(3 * n + 2, 3 * n + 3, 2000 + n + dst) if n == 32 else ref.picture(3 * n + 2, 3 * n + 3,
                                                                                             2000 + n + dst)
    qp = 4 if n == 32 else 22
    modes, lvl, rec, _ = ref.rdo_plane_closed(src, n, qp, dst)
    assert len(np.unique(modes)) >= 3 and np.count_nonzero(lvl) and len(np.unique(rec)) > 2
    assert np.array_equal(dn.decode(modes, lvl, qp, n, dst), rec)


# ---- 4. the shared inputs stay inside their caps ----

@pytest.mark.parametrize("n,dst", dn.KINDS)
def test_every_mode_input_is_not_degenerate(n, dst):
    modes = dn.every_mode(n, dst)[0]
    for pos in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2)):   # corner, first row, first column, interior, last column
        assert sorted(modes[:, pos[0], pos[1]].tolist()) == list(range(35)), pos
    blocks, nonzero, constant, railed = dn.every_mode_census(n, dst)
    print(f"N = {n} dst = {dst}: {nonzero}/{blocks} nonzero residuals, {constant} constant blocks, "
          f"{100 * railed:.1f} % of the samples at 0 or 255")
    assert blocks == 315 and nonzero == blocks and constant == 0 and railed <= dn.RAILED_CAP


@pytest.mark.parametrize("n,dst", dn.KINDS)
def test_wrap_input_tells_the_wrapping_add_from_a_saturating_one(n, dst):
    modes, lvl, qp = dn.wrap_input(n, dst)
    _, _, peak, differ = dn.WRAP[(n, dst)]
    res = dn.residual_plane(lvl, qp, np.zeros(lvl.shape, np.int16), n, dst)
    assert int(res.max()) == peak and peak + 128 > 32767
    wrap = dn.decode(modes, lvl, qp, n, dst)
    sat = dn.decode(modes, lvl, qp, n, dst, reconstruct=dn.saturating_reconstruct)
    d = wrap != sat
    assert int(d.sum()) == differ and not d[:n].any() and not d[:, :n].any()
    assert (wrap[d] == 0).all() and (sat[d] == 255).all()


# ---- C ABI ----

NAMES = ("nh_dequant_inv_planes_n", "nh_intra_decode_closed_n_workspace_bytes", "nh_intra_decode_planes_closed_n")


def test_entry_points_are_exported_and_in_the_signature_table():
    from nano_hevc import _lib
    header = open(os.path.join(ROOT, "include", "nanohevc.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name) and name in header


def test_refusals_precede_any_device_call():
    """Every refusal returns NH_EARG on the host with its text in nh_last_error; the pointers are fakes
    that no device call could survive.  The encoder's refusals minus QP."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    fake = C.c_void_p(1 << 20)
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    sets9 = (PlaneSet * 9)(*([ok] * 9))

    def dec(sets=ok, nsets=1, n=16, dst=0, work=fake):
        arr = sets if not isinstance(sets, PlaneSet) else C.byref(sets)
        return L.nh_intra_decode_planes_closed_n(fake, fake, arr, nsets, n, dst, 30, fake, work, None)

    def deq(sets=ok, nsets=1, n=16, dst=0, lb=4):
        arr = sets if not isinstance(sets, PlaneSet) else C.byref(sets)
        return L.nh_dequant_inv_planes_n(fake, lb, fake, arr, nsets, n, dst, 30, None)

    for call in (dec, deq):
        for n in (0, 2, 5, 12, 64, -4):
            assert call(n=n) == _lib.NH_EARG, n
            assert b"block_size" in L.nh_last_error()
        for n in (8, 16, 32):
            assert call(n=n, dst=1) == _lib.NH_EARG, n
            assert b"use_dst" in L.nh_last_error()
        for n in (4, 8, 16, 32):               # block_size 8 is checked before it is forwarded
            for nsets in (0, -1, 9):
                assert call(sets=sets9, nsets=nsets, n=n) == _lib.NH_EARG, (n, nsets)
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
    for n in (4, 16, 32):
        for lb in (0, 1, 3, 8):
            assert deq(n=n, lb=lb) == _lib.NH_EARG, (n, lb)
            assert b"lvl_bytes" in L.nh_last_error()
        assert dec(n=n, work=C.c_void_p((1 << 20) + 4)) == _lib.NH_EARG, n
        assert b"8-byte" in L.nh_last_error()
    for null in range(5):                  # modes, lvl, sets, recon, work
        args = [fake, fake, C.byref(ok), 1, 16, 0, 30, fake, fake, None]
        args[(0, 1, 2, 7, 8)[null]] = None
        assert L.nh_intra_decode_planes_closed_n(*args) == _lib.NH_EARG, null
        assert b"null" in L.nh_last_error()
    for null in range(3):                  # lvl, res, sets
        args = [fake, 4, fake, C.byref(ok), 1, 16, 0, 30, None]
        args[(0, 2, 3)[null]] = None
        assert L.nh_dequant_inv_planes_n(*args) == _lib.NH_EARG, null
        assert b"null" in L.nh_last_error()


def test_a_qp_outside_0_51_is_not_refused():
    """A decoder clamps QP: with QP 52 or -1 a call whose only fault comes later in the checks -- a level
    size of 3 bytes, a misaligned workspace -- is refused for that fault, not for the QP."""
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    fake, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)
    ok = PlaneSet(0, 0, 0, 64, 64, 64, 1, 1, 0)
    for qp in (52, -1):
        for n in (4, 8, 16, 32):
            assert L.nh_dequant_inv_planes_n(fake, 3, fake, C.byref(ok), 1, n, 0, qp, None) == _lib.NH_EARG, (n, qp)
            err = L.nh_last_error()
            assert b"lvl_bytes" in err and b"qp" not in err, err
        for n in (4, 16, 32):              # N = 8 is forwarded after the argument checks
            assert L.nh_intra_decode_planes_closed_n(fake, fake, C.byref(ok), 1, n, 0, qp, fake, odd,
                                                     None) == _lib.NH_EARG, (n, qp)
            err = L.nh_last_error()
            assert b"8-byte" in err and b"qp" not in err, err


def test_workspace_size_is_the_encoders():
    from nano_hevc import _lib
    from nano_hevc._lib import PlaneSet
    L = _lib.load()
    size, enc = L.nh_intra_decode_closed_n_workspace_bytes, L.nh_intra_rdo_closed_n_workspace_bytes
    sets = (PlaneSet * 2)(PlaneSet(0, 0, 0, 70, 53, 70, 1, 3, 53 * 70), PlaneSet(3 * 53 * 70, 24 * 40, 0, 40, 24, 40, 2, 1, 0))
    for n in (4, 16, 32):
        assert size(sets, 2, n) == enc(sets, 2, n) == 8 + 8 * (3 * (35 + n) + 2 * (20 + n)), n
    assert size(sets, 2, 8) == L.nh_intra_decode_closed_workspace_bytes(sets, 2) > 0
    assert size(None, 1, 16) < 0
    for n in (0, 12, 64):
        assert size(sets, 2, n) < 0, n
    for nsets in (0, 9):
        assert size(sets, nsets, 16) < 0, nsets
    for n in (4, 8, 16, 32):
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 63, 1, 1, 0)), 1, n) < 0, n      # pitch < width
        assert size(C.byref(PlaneSet(0, 0, 0, 64, 64, 64, 0, 1, 0)), 1, n) < 0, n      # no plane per group
    assert size(C.byref(PlaneSet(0, 0, 0, 70000, 64, 70000, 1, 1, 0)), 1, 16) < 0       # wider than 65535
    # any plane set the encoder at N accepts is decodable: an empty plane, a set without groups
    for s in (PlaneSet(0, 0, 0, 0, 64, 0, 1, 1, 0), PlaneSet(0, 0, 0, 64, 0, 64, 1, 1, 0), PlaneSet(0, 0, 0, 64, 64, 64, 1, 0, 0)):
        for n in (4, 16, 32):
            assert size(C.byref(s), 1, n) == enc(C.byref(s), 1, n) >= 8, n
