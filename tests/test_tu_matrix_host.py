"""The fixtures of tests/tu_matrix.py meet their conditions: the geometry of every (ctb, is_luma) case,
the TU census per group and size, the DC / planar / tie outcomes and the narrow / wide group split --
all from the pinned oracle and tu_decode_ref.py on the CPU, so test_tu_matrix_gpu.py's comparisons
exercise what they claim to."""
import numpy as np
import pytest

import tu_decode_ref as R
import tu_matrix as M

CASE_IDS = [c.name for c in M.CASES]


def test_case_table_covers_the_matrix():
    assert sorted((c.ctb, c.luma) for c in M.CASES if not c.name.endswith("-tall")) == \
        sorted((ctb, luma) for ctb in (4, 8, 16, 32) for luma in (True, False))
    tall = M.BY_NAME["ctb4-luma-tall"]
    g = M.geometry(tall)
    assert (tall.w, tall.h, g.strips, g.groups) == (268, 132, 66, 17)
    # the wide pass's second workgroup (16 groups each) has a marked group: the last strip holds a wide sample
    gw = M.group_wide(tall, M.plane(tall, "c"))
    assert gw[16] and "own" in M.strip_reasons(tall, M.plane(tall, "c"))[65]


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_geometry(case):
    g = M.geometry(case)
    assert case.w % 4 == 0 and case.h % 4 == 0
    assert g.strips_x >= 2                                   # two strips across
    assert case.w % g.sw != 0                                # a partial last strip column
    assert case.ctb == 4 or case.h % case.ctb != 0           # a partial last CTU row
    assert g.strips % 4 != 0 and g.groups >= 2               # idle waves in the last group; two groups
    assert case.w <= 268 and case.h <= 136
    for kind in "abcde":
        p = M.plane(case, kind)
        assert p.dtype == np.int16 and p.shape == (case.h, case.w)
    for kind in M.KINDS_8BIT:
        assert M.plane(case, kind).min() >= 0 and M.plane(case, kind).max() <= 255
    assert set(np.unique(M.plane(case, "b")).tolist()) == {0, 255}
    assert M.plane(case, "d").min() < -30000 and M.plane(case, "d").max() > 30000
    e = M.plane(case, "e")
    assert (e[:case.patch[1] * case.ctb, :case.patch[0] * case.ctb] == 128).all()
    assert case.patch[0] * case.ctb <= case.w and case.patch[1] * case.ctb <= case.h


@pytest.mark.parametrize("case", M.CLOSED_ALIGNED, ids=[c.name for c in M.CLOSED_ALIGNED])
def test_closed_aligned_cases(case):
    assert case.w % 8 == 0 and case.h % 4 == 0 and (case.ctb == 4 or case.h % case.ctb)
    assert (case.w - 4) % 8 == 4      # CTB 4: the last CTU of a row starts 4 samples before the row's end
    for kind in M.KINDS_8BIT:
        assert M.plane(case, kind).min() >= 0 and M.plane(case, kind).max() <= 255
    tu = M.reference(case, "a", case.qp, closed=True)[2]
    assert sorted({n for _, _, n in R.tus(tu, case.ctb)}) == M.sizes(case)


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_tu_census(case):
    tu = M.tu_map(case)
    assert R.valid(tu, case.ctb)
    org = M.census(case).origins
    assert int(org.sum()) == len(R.tus(tu, case.ctb))
    assert not org[:, len(M.sizes(case)):].any()
    for k, n in enumerate(M.sizes(case)):
        assert org[:, k].sum() > 0, f"no {n}x{n} TU"
        assert (org[:, k] % M.batch_unit(n) != 0).any(), f"no group with a partial trailing batch of {n}x{n} TUs"
    assert (org[:, 0] > 16).any()                            # 4x4 TUs: more than one batch in a group
    if case.ctb == 32:                                       # two 32x32 TUs per batch on the packed butterflies:
        assert ((org[:, 3] % 2 == 1) & (org[:, 3] >= 1)).any()   # a half-filled batch
        assert (org[:, 3] >= 2).any()                            # and a full one


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_dc_planar_outcomes(case):
    out = M.census(case).outcomes
    for k, n in enumerate(M.sizes(case)):
        eight = sum(out[kind][k] for kind in M.KINDS_8BIT)
        assert (eight > 0).all(), (n, "8-bit planes: DC wins, planar wins, ties", eight.tolist())
        wide = sum(out[kind][k] for kind in M.KINDS_WIDE)
        assert (wide[:2] > 0).all(), (n, "wide planes: DC wins, planar wins", wide.tolist())
        assert out["e"][k][2] > 0, (n, "the constant patch ties")


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_wide_rule(case):
    g = M.geometry(case)
    pl = M.plants(case)
    right, below = M.plant_strips(case)
    values = [v for _, _, v in pl.values()]
    assert any(255 < v < 512 for v in values) and any(v < 0 for v in values)
    assert all(0 <= y < case.h and 0 <= x < case.w for y, x, _ in pl.values())
    assert right % g.strips_x < g.strips_x - 1 and below + g.strips_x < g.strips
    # where each plant lies
    y, x, _ = pl["interior"]
    y0, x0 = M.strip_origin(case, right)
    assert M.strip_at(case, y, x) == right and y0 < y < min(y0 + case.ctb, case.h) - 1 and x0 < x < x0 + g.sw - 1
    y, x, _ = pl["right_edge"]
    assert M.strip_at(case, y, x) == right and M.strip_at(case, y, x + 1) == right + 1
    y, x, _ = pl["bottom_edge"]
    assert M.strip_at(case, y, x) == below and M.strip_at(case, y + 1, x) == below + g.strips_x
    assert pl["last"][:2] == (case.h - 1, case.w - 1)
    # one plant alone: exactly the strips the rule names are wide, each for the one reason
    alone = {"interior": {right: {"own"}}, "right_edge": {right: {"own"}, right + 1: {"left"}},
             "bottom_edge": {below: {"own"}, below + g.strips_x: {"top"}}, "last": {g.strips - 1: {"own"}}}
    for name, want in alone.items():
        for kind in (name, name + "!"):      # the table's value and tu_matrix.FAR
            why = M.strip_reasons(case, M.source(case, kind))
            assert {s: w for s, w in enumerate(why) if w} == want, kind
        assert M.source(case, name + "!")[pl[name][:2]] == M.FAR
    # the strip below lies in another group: that group is wide through a top row alone
    assert below // 4 != (below + g.strips_x) // 4
    gw = M.group_wide(case, M.plane_c_single(case, "bottom_edge"))
    assert [k for k, w in enumerate(gw) if w] == [below // 4, (below + g.strips_x) // 4]
    if case.ctb == 32:   # three strips across: a strip and its right neighbour in two groups
        assert right // 4 != (right + 1) // 4
    # plane c: a narrow group and a wide one; the other planes all narrow / all wide
    gw = M.group_wide(case, M.plane(case, "c"))
    assert any(gw) and not all(gw), gw
    for kind in M.KINDS_8BIT:
        assert not any(M.group_wide(case, M.plane(case, kind)))
    assert all(M.group_wide(case, M.plane(case, "d")))
    mask = M.strip_wide_mask(case, M.plane(case, "c"))
    assert mask.any() and not mask.all()


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_oracle_tells_luma_from_chroma(case):
    """Same plane, plane id and seed: only the 4x4 transform (DST / DCT) differs, and the levels show it."""
    for closed in (False, True):
        for kind in ("a", "c"):
            lu = M.reference(case, kind, case.qp, closed, luma=True)
            ch = M.reference(case, kind, case.qp, closed, luma=False)
            assert np.array_equal(lu[2], ch[2])
            assert not np.array_equal(lu[0], ch[0]), (closed, kind)
            four = np.repeat(np.repeat(lu[2] == 2, 4, axis=0), 4, axis=1)
            if not closed:   # open loop: TUs are independent, so only the 4x4 TUs differ
                assert np.array_equal(lu[0][~four], ch[0][~four]) and np.array_equal(lu[1][~four], ch[1][~four])


def test_valid_keeps_its_answers():
    """``tu_decode_ref.valid`` at ctb 4 / 8, and unchanged at 16 / 32."""
    for case in M.CASES:
        tu = M.tu_map(case)
        assert R.valid(tu, case.ctb)
    assert not R.valid(np.full((4, 4), 3, np.uint8), 4) and R.valid(np.full((4, 4), 2, np.uint8), 4)
    assert R.valid(np.full((4, 4), 3, np.uint8), 8) and not R.valid(np.full((4, 4), 4, np.uint8), 8)
    assert R.valid(np.full((4, 4), 4, np.uint8), 16) and not R.valid(np.full((8, 8), 5, np.uint8), 16)
    assert R.valid(np.full((8, 8), 5, np.uint8), 32) and not R.valid(np.full((8, 8), 1, np.uint8), 32)
