"""The yardstick of config 4's TU-size search and map-driven encode (DESIGN.md §3.4a;
tests/tu_rd_ref.py) checked on the CPU: it reproduces the reference-composed records,
ties in with the pinned oracle's seeded pipeline, finds the optimum over all
quadtrees, lets the parent win ties, and its fixtures use every TU size."""
import numpy as np
import pytest

from oracle import oracle as O

import tu_decode_ref as R
import tu_rd_ref as T


def test_yardstick_reproduces_the_recorded_search(golden):
    g = golden("tu_rd.npz")
    assert str(g["numpy"]).split(".")[0] == "2"
    assert int(g["ncases"]) == 4
    sizes = set()
    for k in range(4):
        ctb, luma, qp, lam = (int(g[f"c{k}_{n}"]) for n in ("ctb", "luma", "qp", "lam"))
        src = g[f"c{k}_src"]
        assert src.min() >= 0 and src.max() <= 255
        tu, pm, lvl, rec, stats = T.rd_plane(src, ctb, qp, lam, bool(luma))
        for name, got in (("tu", tu), ("pm", pm), ("lvl", lvl), ("rec", rec), ("stats", stats)):
            want = g[f"c{k}_{name}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), (k, name)
        sizes |= {(ctb, int(v)) for v in np.unique(tu)}
    assert sizes == {(32, 2), (32, 3), (32, 4), (32, 5), (16, 2), (16, 3), (16, 4)}


def _wave_picture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = 128 + 60 * np.sin(x / 5 + y / 9) + 40 * np.cos(y / 3 - x / 11) + rng.integers(-6, 7, (h, w))
    return a.clip(0, 255).astype(np.int16)


@pytest.mark.parametrize("ctb,luma,pid", [(16, True, 0), (16, False, 1), (32, True, 0), (32, False, 2)])
def test_encode_map_on_a_seeded_map_is_the_seeded_pipeline(ctb, luma, pid):
    src = _wave_picture(68, 100, 5 + ctb + pid)
    lvl, rec, tu = O.tu_pipeline_plane(src, ctb, pid, 2024, 27, luma)
    assert R.valid(tu, ctb) and len(np.unique(tu)) == int(np.log2(ctb)) - 1   # every size 4 .. ctb
    pm, l, r, stats = T.encode_map(src, tu, ctb, 27, 0, luma)
    assert np.array_equal(l, lvl) and np.array_equal(r, rec)
    assert set(np.unique(pm).tolist()) == {0, 1}


def _all_trees(ch, lam, x, y, s, w, h):
    """J of every admissible quadtree of the node (a node that overhangs the plane splits)."""
    if x >= w or y >= h:
        return [0]
    out = []
    if x + s <= w and y + s <= h:
        _, _, _, d, r = ch(x, y, s)
        out.append(d + lam * r)
    if s > 4:
        kids = [0]
        for dy in (0, s // 2):
            for dx in (0, s // 2):
                kids = [a + b for a in kids for b in _all_trees(ch, lam, x + dx, y + dy, s // 2, w, h)]
        out += kids
    return out


@pytest.mark.parametrize("qp,lam", [(22, 400), (32, 1000)])
def test_search_is_optimal_over_all_17_quadtrees(qp, lam):
    h, w, ctb = 36, 44, 16   # ragged: the last CTB row and column overhang the plane
    src = T.mixed_picture(h, w)
    ch = T.Chains(src, qp, False)
    per = {}
    tu = T.rd_plane(src, ctb, qp, lam, False, chains=ch, per_ctb=per)[0]
    counts = set()
    for (cx, cy), j in per.items():
        trees = _all_trees(ch, lam, cx, cy, ctb, w, h)
        counts.add(len(trees))
        assert min(trees) == j, (cx, cy)
    assert 17 in counts and min(counts) < 17          # whole CTBs and CTBs with forced splits
    assert len(np.unique(tu)) > 1


@pytest.mark.parametrize("ctb", [16, 32])
def test_the_parent_wins_ties(ctb):
    src = np.full((64, 64), 128, np.int16)
    ch = T.Chains(src, 30, True)
    tu, pm, lvl, rec, stats = T.rd_plane(src, ctb, 30, 0, True, chains=ch)
    assert stats[0] == 0 and (tu == int(np.log2(ctb))).all()
    strict = T.rd_plane(src, ctb, 30, 0, True, parent_wins=lambda j, kids: j < kids, chains=ch)[0]
    assert (strict == 2).all()     # the fixture tells <= from <


MIXED = [(True, 132, 164, 32), (False, 68, 84, 16)]


@pytest.fixture(scope="module")
def mixed_runs():
    out = {}
    for luma, h, w, ctb in MIXED:
        src = T.mixed_picture(h, w)
        for qp, lam in T.QP_LAMBDA:
            out[(luma, qp, lam)] = (src, ctb) + T.rd_plane(src, ctb, qp, lam, luma)
    return out


@pytest.mark.parametrize("qp,lam", T.QP_LAMBDA)
@pytest.mark.parametrize("luma", [True, False])
def test_mixed_fixture_uses_every_size(mixed_runs, luma, qp, lam):
    src, ctb, tu, pm, lvl, rec, stats = mixed_runs[(luma, qp, lam)]
    assert R.valid(tu, ctb)
    shares = T.area_shares(tu, ctb)
    assert len(shares) == int(np.log2(ctb)) - 1 and abs(sum(shares) - 1) < 1e-12
    assert min(shares) >= 0.05, shares
    assert set(np.unique(pm).tolist()) == {0, 1}


@pytest.mark.parametrize("luma", [True, False])
def test_outputs_agree_with_stage_r(mixed_runs, luma):
    qp, lam = 22, 400
    src, ctb, tu, pm, lvl, rec, stats = mixed_runs[(luma, qp, lam)]
    res = R.residual(lvl, tu, ctb, qp, luma)
    out = np.zeros_like(rec)
    for x, y, n in R.tus(tu, ctb):
        top, left = T.neighbours(src, x, y, n)
        pred = O.intra_dc(top, left, n) if pm[y // 4, x // 4] else O.intra_planar(top, left, int(top[-1]), int(left[-1]), n)
        out[y:y + n, x:x + n] = O.clip(O.reconstruct(pred, res[y:y + n, x:x + n]), 8)
    assert np.array_equal(out, rec)
    d = int(((src.astype(np.int64) - rec) ** 2).sum())
    r = int(np.count_nonzero(lvl)) + len(R.tus(tu, ctb))
    assert stats.tolist() == [d + lam * r, d, r]
