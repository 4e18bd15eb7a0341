#!/usr/bin/env python3
"""Time of the 35-mode RDO with a rate term (gpu.intra_rdo_rd_planes_n / gpu.intra_rdo_rd_closed_n,
DESIGN.md §4.3f) on one MI355X, against the distortion-only entry points at the same N in the same run.

Workload: the streams of tools/bench_rdo_n.py and tools/bench_rdo_closed_n.py -- 1080p YUV420
frames (synthetic content resident in HBM), luma and chroma sets at the same N; N = 4 runs DST
on the luma set and DCT on the chroma set.  Open loop: --frames-open frames (16), QP 22 on the
8-bit stream, QP 4 at N = 32.  Closed loop: --frames-closed frames (64), QP 32 on the 8-bit
stream, QP 4 on the wide stream ((picture - 128) * 32 + 128) at N = 32.  The RD calls run at
--lam (the time does not depend on it beyond the decisions it moves).

Per N every repetition alternates, in this process, among the four calls: RD open, existing
open, RD closed, existing closed.  At N = 8 the existing calls are the packed 8x8 kernels
(intra_rdo_planes / intra_rdo_closed) and the RD calls the N-lane chains, so that line is the
price of N = 8's rate term today, not an overhead of the rate term.

Before timing, on 2 frames per N: lam = 0 must equal the existing entry point's modes, levels
and recon (both loops), the RD outputs at --lam must equal the CPU yardstick
(tests/rdo_rd_ref.py) on one small plane, and intra_decode_closed_n must reproduce the closed
RD recon at --lam.

HIP events on the launch stream, warm-up first, medians and ranges; one JSON line per N
appended to --out (default profiles/r13/bench_rdo_rd.jsonl).
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

from bench_rdo_closed_n import timed_round  # noqa: E402
from bench_rdo_n import W, H, synth_stream  # noqa: E402


def check_against_yardstick(gpu):
    """Both RD calls on one small plane per kind at the table's lambda: every output bit-exact."""
    import rdo_rd_ref as ref
    for n, dst in ref.KINDS:
        _, qp, lam = ref.TABLE[(n, dst)]
        src = ref.table_picture(n, dst)
        h, w = src.shape
        d = torch.from_numpy(src.ravel().copy()).cuda()
        for fn, walk in ((gpu.intra_rdo_rd_planes_n, ref.rd_plane), (gpu.intra_rdo_rd_closed_n, ref.rd_plane_closed)):
            m, l, r, s = fn(d, [gpu.plane_set(0, w, h)], n, qp, lam, dst)
            torch.cuda.synchronize()
            wm, wl, wr, ws, _ = walk(src, n, qp, lam, dst)
            full = np.s_[:h // n * n, :w // n * n]
            assert np.array_equal(m.cpu().numpy(), wm.ravel()), (n, dst)
            assert np.array_equal(l.cpu().numpy().reshape(h, w)[full], wl[full]), (n, dst)
            assert np.array_equal(r.cpu().numpy().reshape(h, w)[full], wr[full]) and s[0].tolist() == list(ws), (n, dst)


def check_on_stream(gpu, n, src, sets, qp_open, qp_closed, lam):
    """lam = 0 equals the existing entry points; the decoder reproduces the closed RD recon."""
    parts = [(sets[:1], True), (sets[1:], False)] if n == 4 else [(sets, False)]
    for ss, dst in parts:
        a = gpu.intra_rdo_rd_planes_n(src, ss, n, qp_open, 0, dst)
        b = gpu.intra_rdo_planes_n(src, ss, n, qp_open, dst)
        c = gpu.intra_rdo_rd_closed_n(src, ss, n, qp_closed, 0, dst)
        e = gpu.intra_rdo_closed_n(src, ss, n, qp_closed, dst)
        torch.cuda.synchronize()
        for x, y in ((a, b), (c, e)):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), (n, dst)
            assert torch.equal(x[3][:, 0], y[3]) and torch.equal(x[3][:, 1], y[3]), (n, dst)
        m, l, r, _ = gpu.intra_rdo_rd_closed_n(src, ss, n, qp_closed, lam, dst)
        assert torch.equal(gpu.intra_decode_closed_n(m, l, ss, n, qp_closed, dst), r), (n, dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-open", type=int, default=16)
    ap.add_argument("--frames-closed", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lam", type=int, default=1000)
    ap.add_argument("--sizes", default="4,8,16,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "bench_rdo_rd.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rdo_rd needs an MI355X"
    from nano_hevc import gpu
    check_against_yardstick(gpu)
    Fo, Fc, lam = a.frames_open, a.frames_closed, a.lam
    buf = synth_stream(max(Fo, Fc))
    wide = ((buf.to(torch.int32) - 128) * 32 + 128).to(torch.int16)
    so, sc, s2 = gpu.yuv420_plane_sets(Fo, W, H), gpu.yuv420_plane_sets(Fc, W, H), gpu.yuv420_plane_sets(2, W, H)
    lvl = torch.zeros(buf.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(buf.shape, dtype=torch.int16, device="cuda")
    dev = torch.cuda.get_device_name(0)

    def split(fn, n, sets, *args):
        """The call over the stream; N = 4: DST on the luma set, DCT on the chroma set."""
        if n == 4:
            def f():
                fn(*args[:1], sets[:1], 4, *args[1:], True, lvl=lvl, rec=rec)
                fn(*args[:1], sets[1:], 4, *args[1:], False, lvl=lvl, rec=rec)
            return f
        return lambda: fn(*args[:1], sets, n, *args[1:], False, lvl=lvl, rec=rec)

    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        qo, qc = (4, 4) if n == 32 else (22, 32)
        src_c = wide if n == 32 else buf
        two = 2 * gpu.yuv420_frame_elems(W, H)
        check_on_stream(gpu, n, buf[:two], s2, qo, qo, lam)
        check_on_stream(gpu, n, src_c[:two], s2, qc, qc, lam)
        fns = [split(gpu.intra_rdo_rd_planes_n, n, so, buf, qo, lam), split(gpu.intra_rdo_planes_n, n, so, buf, qo),
               split(gpu.intra_rdo_rd_closed_n, n, sc, src_c, qc, lam), split(gpu.intra_rdo_closed_n, n, sc, src_c, qc)]
        t = timed_round(fns, a.reps, a.warmup)
        med = [x[len(x) // 2] for x in t]
        ln = {"tool": "bench_rdo_rd", "device": dev, "n": n, "lam": lam, "width": W, "height": H, "reps": a.reps,
              "warmup": a.warmup, "frames_open": Fo, "frames_closed": Fc, "qp_open": qo, "qp_closed": qc,
              "closed_source": "wide" if n == 32 else "8-bit",
              "existing_entry_points": "packed 8x8 kernels" if n == 8 else "the same N-lane kernels, RD = false"}
        for key, k, F in (("rd_open", 0, Fo), ("open", 1, Fo), ("rd_closed", 2, Fc), ("closed", 3, Fc)):
            ln[f"{key}_ms_per_frame"] = round(med[k] / F, 5)
            ln[f"{key}_min_max"] = [round(t[k][0] / F, 5), round(t[k][-1] / F, 5)]
        ln["rd_over_existing_open"] = round(med[0] / med[1], 3)
        ln["rd_over_existing_closed"] = round(med[2] / med[3], 3)
        ln["checks"] = "lam 0 == existing (both loops, 2 frames); decode(closed RD) == rec; yardstick at the table's lambda"
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
