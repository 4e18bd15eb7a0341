"""GPU parity of the 35-mode RDO encoders with EVERY intra mode as the winner (DESIGN.md §3.3a,
§3.7a): the kernels emit only the winning mode's levels and recon, so a mode that never wins on a
test picture has its prediction checked from one side only (its cost must not undercut the winner)
and its store path not at all.  Fixtures: tests/rdo_plant.py, checked on the CPU by
test_rdo_plant_host.py.

A. Planted winners.  Per kind (N = 4 DST, 4 DCT, 8, 16, 32), loop and target block -- (1, 1)
   interior, (1, 2) last full block column, (2, 1) last full block row of a 3 x 3 block plane with
   ragged edges -- one launch whose planes each have another mode planted as the target's only
   winner; rdo_plant.UNPLANTED lists the few modes without a plane.  N = 8 runs twice: all planes
   8-bit (the packed chain) and with one more plane that holds a sample of 300 (closed loop: the
   whole call takes the 32-bit form; open loop: that plane's group takes the general fallback launch).
B. Census.  Per recipe of rdo_plant.CENSUS one noise plane of 16 x 32 blocks on which every mode wins
   a block with levels that are not all zero: the winner's level store under each mode.  There is none
   for the packed open-loop form at N = 8 (8-bit noise lets only 30-31 modes win there); part A covers
   its modes.

Entry points: ``gpu.intra_rdo_planes_n`` / ``intra_rdo_closed_n`` against the yardsticks
rdo_ref.rdo_plane / rdo_closed_ref.rdo_plane_closed, and at N = 8 ``gpu.intra_rdo_planes`` /
``intra_rdo_closed`` directly against the pinned oracle's ``intra_rdo_plane``; never the GPU.  Every
output buffer starts as a sentinel and modes, levels, recon and per-plane SSE are compared bit-exactly
over the whole buffers.  The conditions of each fixture are asserted on the CPU before the launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdo_plant as P  # noqa: E402

PLANTED = [(n, dst, closed, pos, False) for n, dst in P.KINDS for closed in (False, True) for pos in P.POSITIONS] + \
          [(8, False, closed, pos, True) for closed in (False, True) for pos in P.POSITIONS]


@pytest.fixture(scope="module")
def torch():
    import torch
    from nano_hevc import _lib
    assert _lib.device_count() > 0 and torch.cuda.is_available(), "no HIP device: the gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def gpu():
    from nano_hevc import gpu
    return gpu


def _run(torch, gpu, buf, sets, n, qp, dst, closed):
    """One launch on ``buf``, levels and recon pre-filled with the sentinel."""
    ps = [gpu.plane_set(s["base"], s["width"], s["height"], s["pitch"], 1, s["num_groups"], 0, s["group_stride"])
          for s in sets]
    d = torch.from_numpy(buf).cuda()
    lvl = torch.full(buf.shape, P.SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full(buf.shape, P.SENTINEL, dtype=torch.int16, device="cuda")
    if n == 8:
        m, l, r, s = (gpu.intra_rdo_closed if closed else gpu.intra_rdo_planes)(d, ps, qp, lvl=lvl, rec=rec)
    else:
        m, l, r, s = (gpu.intra_rdo_closed_n if closed else gpu.intra_rdo_planes_n)(d, ps, n, qp, dst, lvl=lvl, rec=rec)
    assert l is lvl and r is rec
    torch.cuda.synchronize()
    return m.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()


def _same(got, want, sets, n, closed, what, plane_name):
    """Bit-exact over the whole buffers; a failure names the kind, the loop, the case, the output, the plane
    (its planted mode) and the block with the reference's winner."""
    got = list(got)
    got[1] = np.where(P.unspecified_levels(got[1].size, sets, n, closed), P.SENTINEL, got[1])
    for name, g, w in zip(("modes", "lvl", "rec", "sse"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.flatnonzero(g != w)
        if bad.size:
            i = int(bad[0])
            k, yx, blk, winner = P.locate(name, i, sets, n, want[0])
            where = "outside every plane" if k is None else f"plane {k} ({plane_name(k)})"
            if yx is not None:
                where += f", sample {yx}"
            where += f", block {tuple(blk)} whose winner is mode {winner}" if blk is not None else ""
            pytest.fail(f"{what}: {name} differs at {bad.size} of {w.size} elements, first at {i} = {where}: "
                        f"got {g[i]}, want {w[i]}", pytrace=False)


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: f"{c[0]}{'dst' if c[1] else ''}-{'closed' if c[2] else 'open'}-"
                         f"{c[3][0]}{c[3][1]}{'-wide' if c[4] else ''}")
def test_planted_winners(torch, gpu, case):
    n, dst, closed, pos, wide = case
    qp = P.plant_qp(n)
    what = f"{P.kind_name(n, dst, closed)}, planted at {pos}{', 32-bit / fallback call' if wide else ''}"
    modes, buf, sets = P.planted_launch(n, dst, closed, pos, wide=wide)
    assert tuple(sorted(set(range(35)) - set(modes))) == P.UNPLANTED.get((n, dst, closed, pos), ()), what
    assert sets[0]["num_groups"] == len(modes) and (buf.max() > 255) == (wide or (n == 32 and closed))
    want = P.expected(buf, sets, n, qp, dst, closed)
    y, x = pos[0] * n, pos[1] * n
    for k, (m, lv) in enumerate(zip(modes, P.plane_views(want[1], sets))):   # the reference's winner: the planted mode
        assert want[0][9 * k + 3 * pos[0] + pos[1]] == m, f"{what}: mode {m} does not win its plane's target"
        assert not lv[y:y + n, x:x + n].any(), f"{what}, mode {m}"

    def plane_name(k):
        return f"planted mode {modes[k]}" if k < len(modes) else "the plane with the wide sample"

    _same(_run(torch, gpu, buf, sets, n, qp, dst, closed), want, sets, n, closed, what, plane_name)


@pytest.mark.parametrize("recipe", P.CENSUS, ids=lambda r: f"{r[0]}{'dst' if r[1] else ''}-"
                         f"{'closed' if r[2] else 'open'}-amp{r[3]}-qp{r[4]}")
def test_census_every_mode_wins_with_levels(torch, gpu, recipe):
    """Wide noise reconstructs to 0 or 255 at a large share of the samples (printed, not capped): the
    levels are compared unclipped, so the clip cannot hide an error."""
    n, dst, closed, amp, qp = recipe
    src, sets, want, counts, railed = P.census(*recipe)
    what = f"{P.kind_name(n, dst, closed)}, census of noise {amp} at QP {qp}"
    print(f"{what}: per-mode minimum {counts.min()} (mode {counts.argmin()}), {100 * railed:.0f} % of the recon "
          f"at 0 or 255")
    assert counts.min() >= 1, f"{what}: modes that never win with levels: {np.flatnonzero(counts == 0)}"
    got = _run(torch, gpu, src.ravel().copy(), sets, n, qp, dst, closed)
    _same(got, want, sets, n, closed, what, lambda k: "the noise plane")
