"""The fixtures of tests/tc32_matrix.py meet their conditions: the block counts and wave pairings of the
geometry cases, the blocks every plant turns wide, the levels each plane reaches at each QP and the
DC / planar / tie outcomes -- all from the pinned oracle and tu_decode_ref.py on the CPU, so
test_tc32_matrix_gpu.py's comparisons exercise what they claim to."""
import numpy as np
import pytest

import tc32_matrix as M

CASE_IDS = [c.name for c in M.CASES]


def test_case_table_and_block_order():
    assert [(c.nbx, c.nby) for c in M.CASES] == [(1, 1), (1, 9), (9, 1), (2, 3), (5, 2), (11, 2)]
    assert (M.PAIRING.nbx, M.PAIRING.nby) == (11, 2)
    # the restated order: wave w of workgroup g codes blocks 8 g + w, then 8 g + w + 4
    assert M.wave_pairs(22)[:4] == [(0, 4), (1, 5), (2, 6), (3, 7)]
    assert M.wave_pairs(22)[8:] == [(16, 20), (17, 21), (18, None), (19, None)]
    assert M.wave_pairs(3) == [(0, None), (1, None), (2, None)] and M.wave_pairs(8)[-1] == (3, 7)
    for n in range(1, 30):
        pairs = M.wave_pairs(n)
        assert sorted(b for p in pairs for b in p if b is not None) == list(range(n))
        for first, second in pairs:
            assert M.wave_of(first) == (first // 8, first % 4, 0)
            assert second is None or M.wave_of(second) == (first // 8, first % 4, 1)
    # per workgroup the number of blocks: exactly 8; 5..7 (waves of two blocks and of one); 1..3 (of one and of none)
    counts = {min(8, M.nblk(c) - 8 * g) for c in M.CASES for g in range(-(-M.nblk(c) // 8))}
    assert 8 in counts and counts & {5, 6, 7} and counts & {1, 2, 3}
    assert 1 in counts                                       # a single block: one wave of one, three of none
    # no block count gives a workgroup waves of two blocks AND of none (tc32_matrix's docstring)
    for n in range(1, 9):
        have = [sum(b is not None for b in p) for p in M.wave_pairs(n)] + [0] * (4 - len(M.wave_pairs(n)))
        assert not (2 in have and 0 in have)
    # wave pairs whose two blocks lie in different block rows
    assert any(s is not None and f // c.nbx != s // c.nbx for c in M.CASES for f, s in M.wave_pairs(M.nblk(c)))


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_geometry(case):
    assert case.w // 32 == case.nbx and case.h // 32 == case.nby
    if case.name != "1x1":
        assert case.w % 32 != 0 and case.h % 32 != 0       # ragged right and bottom edges
    assert case.w * case.h <= 30000
    assert (case.w + 15) // 16 * 16 * case.h <= 30000       # ... also at a 16-element aligned pitch
    for kind in M.KINDS:
        p = M.plane(case, kind)
        assert p.dtype == np.int16 and p.shape == (case.h, case.w)
    for kind in M.KINDS_8BIT:
        assert M.plane(case, kind).min() >= 0 and M.plane(case, kind).max() <= 255
        assert not any(M.block_wide(case, M.plane(case, kind)))
    for kind in ("b", "f"):
        assert set(np.unique(M.plane(case, kind)).tolist()) == {0, 255} or case.name == "1x1"
    f = M.plane(case, "f")
    for b in range(M.nblk(case)):
        y, x = M.block_origin(case, b)
        assert (f[y:y + 32, x:x + 32] == 255 * ((b // case.nbx + b % case.nbx) % 2)).all()
    assert M.plane(case, "d").min() < -30000 and M.plane(case, "d").max() > 30000
    assert all(M.block_wide(case, M.plane(case, "d")))
    e = M.plane(case, "e")
    assert (e[:case.patch[1] * 32, :case.patch[0] * 32] == 128).all()
    assert case.patch[0] <= case.nbx and case.patch[1] <= case.nby


def test_pairing_case_has_every_wave_form():
    case = M.PAIRING
    kinds = ("c",) + M.single_kinds(case)
    assert len(kinds) == 17                                  # all eight plants fit the pairing case
    seen = set()
    for kind in kinds:
        seen |= M.pairings(case, M.source(case, kind))
    assert seen >= {"nn", "nw", "wn", "ww", "n", "w"}, seen
    # plane c alone has all six
    assert M.pairings(case, M.plane(case, "c")) >= {"nn", "nw", "wn", "ww", "n", "w"}
    # a workgroup with no wide block after a workgroup with one
    assert any(a and not b for kind in kinds
               for wg in [M.workgroup_wide(case, M.source(case, kind))] for a, b in zip(wg, wg[1:]))
    # the 8-bit planes: every wave narrow -> narrow; plane d: every wave wide -> wide
    assert M.pairings(case, M.plane(case, "a")) == {"nn", "n"} and M.pairings(case, M.plane(case, "d")) == {"ww", "w"}


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_wide_rule_per_plant(case):
    pl = M.plants(case)
    want_names = {"interior", "last"}
    want_names |= {"right_edge"} if case.nbx >= 2 else set()
    want_names |= {"bottom_edge"} if case.nby >= 2 else set()
    want_names |= {"corner_br", "corner_bl"} if case.nbx >= 2 and case.nby >= 2 else set()
    want_names |= {"partial_col", "partial_row"} if case.name != "1x1" else set()
    assert set(pl) == want_names
    values = [v for _, _, v in pl.values()]
    assert all(-512 < v < 0 or 255 < v < 512 for v in values)            # 9-bit: next to the 8-bit range
    assert any(v > 255 for v in values) and any(v < 0 for v in values)
    assert all(0 <= y < case.h and 0 <= x < case.w for y, x, _ in pl.values())
    # where each plant lies
    y, x, _ = pl["interior"]
    assert 0 < y % 32 < 31 and 0 < x % 32 < 31 and M.block_at(case, y, x) is not None
    assert pl["last"][:2] == (32 * case.nby - 1, 32 * case.nbx - 1)
    if "right_edge" in pl:
        y, x, _ = pl["right_edge"]
        assert x % 32 == 31 and x // 32 < case.nbx - 1 and 0 < y % 32 < 31
    if "bottom_edge" in pl:
        y, x, _ = pl["bottom_edge"]
        assert y % 32 == 31 and y // 32 < case.nby - 1 and 0 < x % 32 < 31
    if "corner_br" in pl:
        y, x, _ = pl["corner_br"]
        assert (y % 32, x % 32) == (31, 31) and y // 32 < case.nby - 1 and x // 32 < case.nbx - 1
        y, x, _ = pl["corner_bl"]
        assert (y % 32, x % 32) == (31, 0) and y // 32 < case.nby - 1 and x // 32 >= 1
    if "partial_col" in pl:
        y, x, _ = pl["partial_col"]
        assert x >= 32 * case.nbx and y < 32 * case.nby and M.block_at(case, y, x) is None
        y, x, _ = pl["partial_row"]
        assert y >= 32 * case.nby and x < 32 * case.nbx and M.block_at(case, y, x) is None
    # one plant alone: exactly the blocks listed for it are wide, each for the one reason; its diagonal
    # (corner plants) or every block (partial-region plants) stays narrow
    for name in pl:
        want, narrow = M.plant_blocks(case, name)
        assert all(0 <= b < M.nblk(case) for b in list(want) + list(narrow))
        if name.startswith("corner"):
            assert len(narrow) >= 1
        for kind in (name, name + "!"):
            src = M.source(case, kind)
            why = M.block_reasons(case, src)
            assert {b: w for b, w in enumerate(why) if w} == want, (kind, why)
            assert not any(M.block_wide(case, src)[b] for b in narrow), kind
            diff = np.argwhere(src != M.plane(case, "a"))
            assert diff.tolist() == [list(pl[name][:2])]
        assert M.source(case, name + "!")[pl[name][:2]] == M.FAR
        # the FAR plant shows: the oracle's outputs differ from plane a's in every block it turns wide through
        # the halo alone (the narrow chain on such a block could not have computed them from 8-bit neighbours)
        for qp in (0, 22):
            la, ra = M.reference(case, "a", qp)
            lf, rf = M.reference(case, name + "!", qp)
            for b, reasons in want.items():
                if "own" not in reasons:
                    y0, x0 = M.block_origin(case, b)
                    assert not np.array_equal(ra[y0:y0 + 32, x0:x0 + 32], rf[y0:y0 + 32, x0:x0 + 32]), (name, b, qp)
                    if qp == 0:
                        assert not np.array_equal(la[y0:y0 + 32, x0:x0 + 32], lf[y0:y0 + 32, x0:x0 + 32]), (name, b)
    # plane c: all the plants
    c = M.plane(case, "c")
    assert len(np.argwhere(c != M.plane(case, "a"))) == len(pl)
    union = set()
    for name in pl:
        union |= set(M.plant_blocks(case, name)[0])
    assert {b for b, w in enumerate(M.block_wide(case, c)) if w} == union
    if M.nblk(case) > 4:
        assert any(M.block_wide(case, c)) and not all(M.block_wide(case, c))


def test_pairing_case_plants_name_the_expected_blocks():
    """Spelled out for the pairing case: block b = 11 * block row + block column."""
    case = M.PAIRING
    want = {"interior": {5}, "right_edge": {0, 1}, "bottom_edge": {9, 20}, "corner_br": {2, 3, 13},
            "corner_bl": {8, 19}, "last": {21}, "partial_col": set(), "partial_row": set()}
    for name, blocks in want.items():
        assert {b for b, w in enumerate(M.block_wide(case, M.source(case, name))) if w} == blocks, name
    assert M.plant_blocks(case, "corner_br")[1] == {14} and M.plant_blocks(case, "corner_bl")[1] == {7, 18}
    wide = M.block_wide(case, M.plane(case, "c"))
    assert [b for b, w in enumerate(wide) if w] == [0, 1, 2, 3, 5, 8, 9, 13, 19, 20, 21]
    assert not wide[18] and wide[19]                         # the lone narrow and the lone wide block


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_levels(case):
    interior = [b for b in range(M.nblk(case)) if b // case.nbx >= 1 and b % case.nbx >= 1]
    for kind in M.KINDS_8BIT:
        for qp in M.QPS + (1,):
            lvl = M.full(case, M.reference(case, kind, qp)[0])
            assert np.abs(lvl).max() <= 51, (kind, qp)
        nz = {qp: int(np.count_nonzero(M.full(case, M.reference(case, kind, qp)[0]))) for qp in M.QPS}
        assert nz[0] > 0, kind
        assert nz[51] == 0, kind
        if kind in ("b", "f"):
            assert nz[4] > 0, kind
        if kind == "f":
            assert nz[22] > 0
    if not interior:   # no block with both neighbours inside the plane: the bound is out of reach (tc32_matrix's docstring)
        assert case.name in ("1x1", "1x9", "9x1") and np.abs(M.full(case, M.reference(case, "f", 0)[0])).max() < 51
    else:              # plane f: +51 and -51 at QP 0, on interior blocks; the ladder of levels on such a block
        l0 = M.full(case, M.reference(case, "f", 0)[0])
        assert l0.max() == 51 and l0.min() == -51
        f = M.plane(case, "f")
        for b in interior:
            y, x = M.block_origin(case, b)
            sign = 1 if f[y, x] == 255 else -1
            for qp, peak in ((0, 51), (1, 45), (4, 32), (22, 4), (51, 0)):
                assert M.reference(case, "f", qp)[0][y, x] == sign * peak, (b, qp)
    # at QP 51 the recon is the chosen prediction
    for kind in M.KINDS_8BIT:
        rec = M.reference(case, kind, 51)[1]
        for b, (e_dc, e_pl) in enumerate(M.census(case, kind)):
            y, x = M.block_origin(case, b)
            dc, planar = M.predictions(case, kind, b)
            assert np.array_equal(rec[y:y + 32, x:x + 32], np.clip(dc if e_dc <= e_pl else planar, 0, 255)), (kind, b)
    # plane d has levels at QP 3 that no int8 holds: they must come back from the spill plane
    assert np.abs(M.full(case, M.reference(case, "d", 3)[0])).max() > 127


@pytest.mark.parametrize("case", M.CASES, ids=CASE_IDS)
def test_dc_planar_outcomes(case):
    eight = np.sum([M.outcomes(case, kind) for kind in M.KINDS_8BIT], axis=0)
    if case.name == "1x1":     # the one block has all its neighbours outside the plane: always a tie
        assert eight.tolist() == [0, 0, 4]
        return
    assert (eight > 0).all(), ("8-bit planes: DC wins, planar wins, ties", eight.tolist())
    e = M.census(case, "e")
    for by in range(case.patch[1]):
        for bx in range(case.patch[0]):
            assert e[by * case.nbx + bx] == (0, 0)           # the patch ties (with identical predictions)
    # the constructed tie: equal energies, different predictions, DC coded; at QP 51 the recon shows the choice
    bx, by = case.tie
    b = by * case.nbx + bx
    assert (bx, by) != (0, 0) and not (bx < case.patch[0] and by < case.patch[1])
    e_dc, e_pl = e[b]
    assert e_dc == e_pl > 0
    dc, planar = M.predictions(case, "e", b)
    t, l, c = M.tie_params(case)
    yy, xx = np.mgrid[0:32, 0:32]
    assert (dc == c).all() and np.array_equal(planar, c + xx - yy)
    y, x = M.block_origin(case, b)
    rec = M.reference(case, "e", 51)[1][y:y + 32, x:x + 32]
    assert np.array_equal(rec, dc) and not np.array_equal(rec, planar)
    assert int(np.count_nonzero(rec != planar)) == 32 * 31


def test_describe_names_the_block():
    case = M.PAIRING
    src = M.plane(case, "c")
    want = M.reference(case, "c", 22)[1]
    assert M.describe(case, "rec", want, want, src) is None
    got = want.copy()
    got[40, 300] ^= 1                                        # block 11 + 9 = 20
    got[70, 3] ^= 1                                          # in the partial row
    msg = M.describe(case, "rec", got, want, src)
    assert "11x2: rec differs at 2 of" in msg and "(y 40, x 300)" in msg
    assert "block 20 (workgroup 2, wave 0, its second block; wide by the rule)" in msg
    msg = M.describe(case, "lvl", got[64:], want[64:], src, at=(64, 0))
    assert "(y 70, x 3)" in msg and "outside the full blocks" in msg
    assert "shape" in M.describe(case, "rec", got[1:], want, src)


def test_layout_masks():
    case = M.BY_NAME["5x2"]
    lay = M.layout(case, 32, 176, 3, 2, gap=16, group_gap=48)
    offs = M.plane_offsets(lay, 3, 2)
    assert offs[0] == 32 and offs[1] - offs[0] == 72 * 176 + 16 and offs[3] - offs[0] == 3 * (72 * 176 + 16) + 48
    assert lay.size == offs[5] + 72 * 176 + 16 + 48
    out = M.outside_full_mask(case, lay, offs)
    assert int((~out).sum()) == 6 * 64 * 160
    assert out[:32].all() and out[offs[0] + 160] and not out[offs[0] + 159] and out[offs[0] + 64 * 176]
    kinds = ("a", "c", "d", "e", "f", "right_edge!")
    wide = M.wide_full_mask(case, lay, offs, kinds)
    assert not (wide & out).any()
    assert int(wide.sum()) == 1024 * sum(sum(M.block_wide(case, M.source(case, k))) for k in kinds)
