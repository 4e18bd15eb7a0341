#!/usr/bin/env python3
"""Time of the NxN 35-mode CLOSED-loop RDO (gpu.intra_rdo_closed_n) on one MI355X.

Workload: a stream of --frames 1080p YUV420 frames (synthetic content resident in
HBM), luma and chroma sets at the same N, through intra_rdo_closed_n at N = 4
(DST on the luma set, DCT on the chroma set), 16 and 32.  QP 32 on the 8-bit
stream at N = 4 / 16; QP 4 on the wide stream ((picture - 128) * 32 + 128) at
N = 32, where an 8-bit source reconstructs to a constant.

Every repetition alternates, in this process, among four calls: the closed call
at N, the open-loop call at the same N on the same stream, and the N = 8 closed
/ open pair on the 8-bit stream at QP 32.  Target (not a correctness condition):
closed / open at N <= 1.5 x closed / open at N = 8 of the same run.

HIP events on the launch stream, warm-up first, medians and ranges; one JSON
line per N appended to --out (default profiles/r10/bench_rdo_closed_n.jsonl).
Before timing, the closed outputs at each N are compared with the CPU yardstick
(tests/rdo_closed_ref.py) on one small plane.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-hevc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_rdo_n import W, H, synth_stream  # noqa: E402


def check_against_yardstick(gpu):
    """The closed call on one small plane per (N, transform): modes, levels, recon and SSE bit-exact."""
    import rdo_closed_ref as ref
    for n, dst in ((4, True), (4, False), (16, False), (32, False)):
        h, w = 3 * n + 2, 4 * n + 3
        src = ref.wide_picture(h, w, 40 + n) if n == 32 else ref.picture(h, w, 40 + n)
        qp = 4 if n == 32 else 32
        m, l, r, s = gpu.intra_rdo_closed_n(torch.from_numpy(src.ravel().copy()).cuda(), [gpu.plane_set(0, w, h)], n, qp, dst)
        torch.cuda.synchronize()
        wm, wl, wr, ws = ref.rdo_plane_closed(src, n, qp, dst)
        assert np.array_equal(m.cpu().numpy(), wm.ravel()) and np.array_equal(l.cpu().numpy(), wl.ravel()), (n, dst)
        assert np.array_equal(r.cpu().numpy(), wr.ravel()) and int(s[0]) == ws, (n, dst)


def timed_round(fns, reps, warmup):
    """Per function the sorted times (ms) of ``reps`` calls, the functions alternating (a, b, c, d, a, ...)."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
    for e in evs:
        e[0].record(st)
        for k, f in enumerate(fns):
            f()
            e[k + 1].record(st)
    torch.cuda.synchronize()
    return [sorted(e[k].elapsed_time(e[k + 1]) for e in evs) for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="4,16,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "bench_rdo_closed_n.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rdo_closed_n needs an MI355X"
    from nano_hevc import gpu
    check_against_yardstick(gpu)
    F = a.frames
    buf = synth_stream(F)
    wide = ((buf.to(torch.int32) - 128) * 32 + 128).to(torch.int16)
    sets = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(buf.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(buf.shape, dtype=torch.int16, device="cuda")
    dev = torch.cuda.get_device_name(0)

    def calls(n):
        src, qp = (wide, 4) if n == 32 else (buf, 32)
        if n == 4:   # DST luma, DCT chroma
            def closed():
                gpu.intra_rdo_closed_n(src, sets[:1], 4, qp, True, lvl=lvl, rec=rec)
                gpu.intra_rdo_closed_n(src, sets[1:], 4, qp, False, lvl=lvl, rec=rec)

            def opened():
                gpu.intra_rdo_planes_n(src, sets[:1], 4, qp, True, lvl=lvl, rec=rec)
                gpu.intra_rdo_planes_n(src, sets[1:], 4, qp, False, lvl=lvl, rec=rec)
            return closed, opened, qp
        return (lambda: gpu.intra_rdo_closed_n(src, sets, n, qp, False, lvl=lvl, rec=rec),
                lambda: gpu.intra_rdo_planes_n(src, sets, n, qp, False, lvl=lvl, rec=rec), qp)

    def closed8():
        gpu.intra_rdo_closed(buf, sets, 32, lvl=lvl, rec=rec)

    def open8():
        gpu.intra_rdo_planes(buf, sets, 32, lvl=lvl, rec=rec)

    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        closed, opened, qp = calls(n)
        tc, to, tc8, to8 = timed_round([closed, opened, closed8, open8], a.reps, a.warmup)

        def med(t):
            return t[len(t) // 2]
        ratio, ratio8 = med(tc) / med(to), med(tc8) / med(to8)
        ln = {"tool": "bench_rdo_closed_n", "device": dev, "n": n, "qp": qp, "frames": F, "width": W, "height": H,
              "source": "wide" if n == 32 else "8-bit", "reps": a.reps, "warmup": a.warmup,
              "closed_ms_per_frame": round(med(tc) / F, 5), "closed_min_max": [round(tc[0] / F, 5), round(tc[-1] / F, 5)],
              "open_ms_per_frame": round(med(to) / F, 5), "open_min_max": [round(to[0] / F, 5), round(to[-1] / F, 5)],
              "n8_closed_ms_per_frame": round(med(tc8) / F, 5),
              "n8_closed_min_max": [round(tc8[0] / F, 5), round(tc8[-1] / F, 5)],
              "n8_open_ms_per_frame": round(med(to8) / F, 5),
              "n8_open_min_max": [round(to8[0] / F, 5), round(to8[-1] / F, 5)],
              "closed_over_open": round(ratio, 3), "n8_closed_over_open": round(ratio8, 3),
              "target": "closed_over_open <= 1.5 * n8_closed_over_open", "target_met": bool(ratio <= 1.5 * ratio8)}
        if n == 4:
            ln["transforms"] = "DST luma, DCT chroma"
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
