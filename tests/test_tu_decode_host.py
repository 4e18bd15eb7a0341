"""The config-4 decoder's CPU-side checks: the yardstick
``tu_decode_ref`` against the reference's own recorded config-4 closed-loop outputs,
its map-validity rule, the new C-ABI symbols and their host-side argument checks
(before any device call)."""
import ctypes as C

import numpy as np
import pytest

import tu_decode_ref as R

NEW = ("nh_tu_closed_pred_map", "nh_dequant_inv_tu_planes", "nh_tu_decode_closed_workspace_bytes",
       "nh_tu_decode_planes_closed")


@pytest.mark.parametrize("tag", ["k4y", "k4u", "k4n"])
def test_ref_reproduces_recorded_recon(golden, tag):
    """Guards the yardstick (passes without the feature): the map derived from the
    recorded (src, rec, tu) and the recorded levels decode to the recorded recon."""
    g = golden("closed4.npz")
    ctb, qp, luma = int(g[tag + "_ctb"]), int(g[tag + "_qp"]), bool(g[tag + "_luma"])
    tu = g[tag + "_tu"]
    assert R.valid(tu, ctb)
    pm = R.pred_map(g[tag + "_src"], g[tag + "_rec"], tu, ctb)
    assert set(np.unique(pm)) <= {0, 1} and (tag == "k4u" or len(np.unique(pm)) == 2)   # k4u: DC everywhere
    assert np.array_equal(R.decode(tu, pm, g[tag + "_lvl"], ctb, qp, luma), g[tag + "_rec"])
    # the map matters: the other choice everywhere gives another picture
    assert not np.array_equal(R.decode(tu, 1 - pm, g[tag + "_lvl"], ctb, qp, luma), g[tag + "_rec"])


def test_ref_stage_r_is_the_decoders_residual(golden):
    g = golden("closed4.npz")
    tu, lvl = g["k4n_tu"], g["k4n_lvl"]
    res = R.residual(lvl, tu, 32, 22, True)
    sizes = {n for _, _, n in R.tus(tu, 32)}
    assert sizes == {4, 8, 16, 32}
    x, y, n = next(t for t in R.tus(tu, 32) if t[2] == 4 and lvl[t[1]:t[1] + 4, t[0]:t[0] + 4].any())
    blk = lvl[y:y + 4, x:x + 4]
    assert np.array_equal(res[y:y + 4, x:x + 4], R.residual_tu(blk, 22, True))
    assert not np.array_equal(R.residual_tu(blk, 22, True), R.residual_tu(blk, 22, False))   # luma 4x4 is the DST


def _uniform(h4, w4, v):
    return np.full((h4, w4), v, np.uint8)


def test_validity_rule_on_hand_made_maps():
    assert R.valid(_uniform(8, 16, 2), 32) and R.valid(_uniform(8, 16, 3), 32)
    assert R.valid(_uniform(8, 16, 4), 32) and R.valid(_uniform(8, 16, 5), 32)
    assert R.valid(_uniform(8, 16, 4), 16) and not R.valid(_uniform(8, 16, 5), 16)   # 32x32 TU under CTB 16
    assert R.valid(_uniform(5, 9, 2), 32)                  # 20 x 36: only 4x4 fits everywhere
    assert not R.valid(_uniform(5, 9, 3), 32)              # 8x8 TUs cross the right and bottom edges
    mixed = _uniform(8, 8, 2)
    mixed[0:4, 4:8] = 4
    mixed[4:6, 0:2] = 3
    assert R.valid(mixed, 32)
    assert [t for t in R.tus(mixed, 32) if t[2] > 4] == [(16, 0, 16), (0, 16, 8)]
    for v in (0, 1, 6, 255):
        bad = _uniform(8, 8, 2)
        bad[3, 5] = v
        assert not R.valid(bad, 32), v
    lone = _uniform(8, 8, 2)
    lone[2, 2] = 3                                         # one 8x8 unit among 4x4s
    assert not R.valid(lone, 32)
    hole = _uniform(8, 8, 3)
    hole[1, 0] = 2                                         # a valid-looking 4x4 inside an 8x8 square
    assert not R.valid(hole, 32)
    shifted = _uniform(8, 8, 2)
    shifted[1:3, 1:3] = 3                                  # an 8x8 square that is not aligned
    assert not R.valid(shifted, 32)
    edge = _uniform(6, 8, 2)
    edge[4:6, 0:4] = 4                                     # a 16x16 TU reaching below a 24-row plane
    assert not R.valid(edge, 32)


def _lib_and_types():
    from nano_hevc import _lib
    return _lib, _lib.load(), _lib.PlaneSet


def test_new_symbols_exported():
    _lib, L, _ = _lib_and_types()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    from nano_hevc import gpu
    for f in ("tu_pred_map_closed", "dequant_inv_tu", "tu_decode_closed", "tu_decode_closed_yuv420"):
        assert callable(getattr(gpu, f)), f


FAKE = C.c_void_p(1 << 20)   # never dereferenced: the checks return first
OK = (0, 0, 0, 64, 64, 64, 1, 1, 0)
BAD_SIZE = {"width 66": (0, 0, 0, 66, 64, 66, 1, 1, 0), "height 62": (0, 0, 0, 64, 62, 64, 1, 1, 0),
            "width 70, height 45": (0, 0, 0, 70, 45, 70, 1, 1, 0)}
BAD_SETS = {"pitch<width": (0, 0, 0, 64, 64, 56, 1, 1, 0), "width 0": (0, 0, 0, 0, 64, 64, 1, 1, 0),
            "planes 0": (0, 0, 0, 64, 64, 64, 0, 1, 0), "groups<0": (0, 0, 0, 64, 64, 64, 1, -1, 0)}


def _entry_points(L, ps):
    """name -> (callable(set, ctb) with fake pointers, callables with one pointer nulled)."""
    s = C.byref(ps)
    pm = lambda src=FAKE, rec=FAKE, tu=FAKE, st=s, out=FAKE, ctb=32: \
        L.nh_tu_closed_pred_map(src, rec, tu, st, ctb, out, None)
    sr = lambda lvl=FAKE, res=FAKE, tu=FAKE, st=s, ctb=32, lb=4: \
        L.nh_dequant_inv_tu_planes(lvl, lb, res, tu, st, ctb, 1, 30, None)
    de = lambda tu=FAKE, pmap=FAKE, lvl=FAKE, st=s, rec=FAKE, work=FAKE, ctb=32: \
        L.nh_tu_decode_planes_closed(tu, pmap, lvl, st, ctb, 1, 30, rec, work, None)
    return {"pred_map": (pm, ("src", "rec", "tu", "st", "out")), "stage_r": (sr, ("lvl", "res", "tu", "st")),
            "decode": (de, ("tu", "pmap", "lvl", "st", "rec", "work"))}


def test_host_checks_precede_any_device_call():
    _lib, L, PlaneSet = _lib_and_types()
    for name, (f, ptrs) in _entry_points(L, PlaneSet(*OK)).items():
        for ctb in (0, 8, 24, 64, -32):
            assert f(ctb=ctb) == _lib.NH_EARG, (name, ctb)
            assert b"ctb" in L.nh_last_error(), (name, ctb)
        for p in ptrs:
            assert f(**{p: None}) == _lib.NH_EARG, (name, p)
            assert b"null" in L.nh_last_error(), (name, p)
    for what, fields in BAD_SIZE.items():
        for name, (f, _) in _entry_points(L, PlaneSet(*fields)).items():
            for ctb in (16, 32):
                assert f(ctb=ctb) == _lib.NH_EARG, (name, what)
                assert b"multiples of 4" in L.nh_last_error(), (name, what)
    for what, fields in BAD_SETS.items():
        for name, (f, _) in _entry_points(L, PlaneSet(*fields)).items():
            assert f() == _lib.NH_EARG, (name, what)
            assert b"plane set" in L.nh_last_error(), (name, what)
    sr = _entry_points(L, PlaneSet(*OK))["stage_r"][0]
    for lb in (0, 1, 3, 8):
        assert sr(lb=lb) == _lib.NH_EARG
        assert b"lvl_bytes" in L.nh_last_error()
    de = _entry_points(L, PlaneSet(*OK))["decode"][0]
    assert de(work=C.c_void_p((1 << 20) + 4)) == _lib.NH_EARG
    assert b"8-byte" in L.nh_last_error()


def test_workspace_bytes():
    _lib, L, PlaneSet = _lib_and_types()
    f = L.nh_tu_decode_closed_workspace_bytes
    one = f(C.byref(PlaneSet(*OK)), 32)
    assert one >= 16 + 8 * 32 and one % 16 == 0        # status block + one tagged word per sample pair
    four = f(C.byref(PlaneSet(0, 64 * 64, 2 * 64 * 64, 64, 64, 64, 2, 2, 0)), 16)
    assert four - 16 == 4 * (one - 16)                   # a line per plane
    assert f(C.byref(PlaneSet(*OK)), 8) < 0 and f(None, 32) < 0
    for fields in list(BAD_SIZE.values()) + list(BAD_SETS.values()):
        assert f(C.byref(PlaneSet(*fields)), 32) < 0, fields
