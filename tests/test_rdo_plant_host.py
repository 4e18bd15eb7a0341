"""CPU checks of tests/rdo_plant.py, the fixtures that make every one of the 35 intra modes the
RDO winner for test_rdo_modes_gpu.py:

* every planted case meets its conditions -- mode m alone has the lowest cost of the target block,
  whose reference samples are not flat -- re-derived here from the planted plane, and through the
  references' own plane functions for a sample of the cases (all of them at N = 8);
* the modes that could not be planted are exactly rdo_plant.UNPLANTED: none at (1, 1) and (1, 2);
* a predictor that is wrong for mode m only (+2 on every sample) changes the expected outputs of
  m's plane: the fixture notices an error of mode m;
* every census recipe has all 35 modes winning a block with levels that are not all zero;
* the launches are laid out as their docstring says."""
import numpy as np
import pytest

import rdo_closed_ref
import rdo_plant as P
import rdo_ref
from oracle import oracle as O

CASES = [(n, dst, closed, pos) for n, dst in P.KINDS for closed in (False, True) for pos in P.POSITIONS]


def _id(c):
    return f"{c[0]}{'dst' if c[1] else ''}-{'closed' if c[2] else 'open'}-{c[3][0]}{c[3][1]}"


@pytest.fixture
def wrong_mode(monkeypatch):
    """Both yardsticks' predictors with 2 added to every sample of mode ``cell[0]`` (None: unchanged)."""
    cell = [None]
    for mod in (rdo_ref, rdo_closed_ref):
        def bad(plane, x, y, n, mode, good=mod.predict):
            p = good(plane, x, y, n, mode)
            return (p + 2).astype(np.int16) if mode == cell[0] else p
        monkeypatch.setattr(mod, "predict", bad)
    return cell


def _yardstick(src, n, qp, dst, closed):
    return (rdo_closed_ref.rdo_plane_closed if closed else rdo_ref.rdo_plane)(src, n, qp, dst)


def _differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_planted_cases(case, wrong_mode):
    """Conditions 1-3 of every planted case from its plane alone, the unplanted set, and the wrong
    predictor.  With mode m's prediction off by 2 only m's chain changes (the patch leaves the other
    modes alone), so the target's outcome is re-derived from the 34 kept chains and m's new one.  In
    closed loop the neighbours are those of the unpatched walk: either a raster-earlier block changes
    under the patch, and the plane's outputs with it, or none does and the target sees these very
    neighbours -- so a changed outcome of the target means changed outputs of the plane either way.
    One mode per case goes through the yardstick's plane function as well, patched and not."""
    n, dst, closed, pos = case
    qp, name = P.plant_qp(n), f"{P.kind_name(n, dst, closed)}, target {pos}"
    found = P.planted(n, dst, closed, pos)
    missing = tuple(sorted(set(range(35)) - set(found)))
    assert missing == P.UNPLANTED.get(case, ()), f"{name}: modes not planted {missing}"
    assert len(missing) <= 3 and (pos == (2, 1) or not missing)
    y, x = pos[0] * n, pos[1] * n
    walks = {}
    for m, (seed, src) in found.items():
        label = f"{name}, mode {m}, seed {seed}"
        assert P.plant_seed(0) <= seed < P.plant_seed(P.MAX_SEEDS) and src.shape == P.plane_shape(n)
        pic = P.plant_picture(n, closed, seed)
        rest = np.ones(src.shape, bool)
        rest[y:y + n, x:x + n] = False
        assert np.array_equal(src[rest], pic[rest]), label            # only the target block is overwritten
        if seed not in walks:
            walks[seed] = P.neighbour_plane(pic, n, qp, dst, closed, pos)
        nb = walks[seed] if closed else src
        assert not P.references_flat(nb, n, pos, closed), label
        assert np.array_equal(src[y:y + n, x:x + n], P.predict(nb, x, y, n, m, closed)), label
        chains = P.target_chains(src, nb, n, qp, dst, closed, pos)
        costs = [c[2] for c in chains]
        assert P.wins_alone(costs, m), f"{label}: costs {costs}"
        good = P.target_outcome(chains)
        assert good[0] == m and not good[1].any(), label
        wrong_mode[0] = m
        orig = np.ascontiguousarray(src[y:y + n, x:x + n])
        chains[m] = rdo_ref.chain(orig, P.predict(nb, x, y, n, m, closed), qp, n, dst)
        wrong_mode[0] = None
        bad = P.target_outcome(chains)
        assert bad[0] != good[0] or bad[3] != good[3] or _differ(bad[1:3], good[1:3]), \
            f"{label}: a prediction off by 2 leaves the target's outcome unchanged"
    # through the plane functions: one mode per case, a different one from case to case
    modes = sorted(found)
    m = modes[(7 * CASES.index(case)) % len(modes)]
    src = found[m][1]
    want = _yardstick(src, n, qp, dst, closed)
    assert want[0][pos] == m and not want[1][y:y + n, x:x + n].any(), f"{name}, mode {m}"
    wrong_mode[0] = m
    assert _differ(_yardstick(src, n, qp, dst, closed), want), f"{name}, mode {m}: the wrong predictor goes unnoticed"
    wrong_mode[0] = None
    if n == 8:      # the GPU's reference at N = 8 is the oracle's driver: it agrees on every planted plane
        assert not _differ(O.intra_rdo_plane(src, qp, closed=closed), want)
        for m, (_, src) in found.items():
            om, ol, _, _ = O.intra_rdo_plane(src, qp, closed=closed)
            assert om[pos] == m and not ol[y:y + n, x:x + n].any(), f"{name}, mode {m}"


def test_the_unplanted_modes_are_few_and_only_in_the_last_block_row():
    assert all(k in CASES and k[3] == (2, 1) and 0 < len(v) <= 3 for k, v in P.UNPLANTED.items())


@pytest.mark.parametrize("recipe", P.CENSUS, ids=lambda r: f"{r[0]}{'dst' if r[1] else ''}-"
                         f"{'closed' if r[2] else 'open'}-amp{r[3]}-qp{r[4]}")
def test_census_recipes(recipe):
    """Every mode wins at least one of the 512 blocks with levels that are not all zero."""
    n, dst, closed, amp, qp = recipe
    src, sets, want, counts, railed = P.census(*recipe)
    assert src.shape == (16 * n, 32 * n) and want[0].size == 512
    assert (src.min() >= 0 and src.max() <= 255) == (amp == 255)      # 8-bit: the packed chains at N = 8
    print(f"{P.kind_name(n, dst, closed)}, noise {amp}, QP {qp}: per-mode minimum {counts.min()} (mode "
          f"{counts.argmin()}), {counts.sum()} of 512 blocks coded, {100 * railed:.0f} % of the recon at 0 or 255")
    assert counts.min() >= 1, f"modes that never win with levels: {np.flatnonzero(counts == 0)}"


def test_there_is_a_census_of_every_kind_and_loop_but_the_packed_open_8():
    have = {(n, dst, closed) for n, dst, closed, _, _ in P.CENSUS}
    assert have == {(n, dst, closed) for n, dst in P.KINDS for closed in (False, True)}
    assert {(amp, qp) for n, _, closed, amp, qp in P.CENSUS if n == 8 and closed} == {(255, 10), (1000, 22)}
    assert not [r for r in P.CENSUS if r[0] == 8 and not r[2] and r[3] == 255]


@pytest.mark.parametrize("pos", P.POSITIONS)
@pytest.mark.parametrize("n,wide", [(4, False), (8, False), (8, True), (32, False)])
def test_launch_layouts(n, wide, pos):
    modes, buf, sets = P.planted_launch(n, False, True, pos, wide=wide)
    found = P.planted(n, False, True, pos)
    assert modes == sorted(found) and sets[0]["num_groups"] == len(modes) and len(sets) == 1 + wide
    aligned = all(sets[0][k] % 8 == 0 for k in ("base", "pitch", "group_stride"))
    assert aligned == (pos != (1, 2))
    used = np.zeros(buf.size, np.int32)
    for v in P.plane_views(used, sets):
        v += 1
    assert used.max() == 1 and (used == 0).sum() > len(modes)         # disjoint planes, gaps between them
    views = list(P.plane_views(buf, sets))
    for v, m in zip(views, modes):
        assert np.array_equal(v, found[m][1])
    planted_are_8_bit = all(v.min() >= 0 and v.max() <= 255 for v in views[:len(modes)])
    assert planted_are_8_bit == (n != 32)
    if wide:
        assert (views[-1] > 255).sum() == 1 and views[-1].max() == P.WIDE_SAMPLE
    # locate: the target's first sample of plane 3, and the words for the other outputs
    s = sets[0]
    y, x = pos[0] * n, pos[1] * n
    want_modes = np.concatenate([np.full(9, m, np.uint8) for m in modes] + [np.zeros(4, np.uint8)] * wide)
    i = s["base"] + 3 * s["group_stride"] + y * s["pitch"] + x
    assert P.locate("rec", i, sets, n, want_modes) == (3, (y, x), pos, modes[3])
    assert P.locate("lvl", s["base"] + 3 * n * s["pitch"], sets, n, want_modes) == (0, (3 * n, 0), None, None)
    assert P.locate("modes", 9 * 3 + 3 * pos[0] + pos[1], sets, n, want_modes) == (3, None, pos, modes[3])
    assert P.locate("sse", 3, sets, n, want_modes) == (3, None, None, None)
    assert P.locate("rec", 0, sets, n, want_modes) == (None, None, None, None)
