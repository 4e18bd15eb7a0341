#!/usr/bin/env python3
"""Time of the closed-loop intra decoder at N = 4, 16, 32 (gpu.intra_decode_closed_n)
on one MI355X, next to the closed encoder whose outputs it decodes.

Workload: bench_rdo_closed_n.py's -- a stream of --frames 1080p YUV420 frames
(synthetic content resident in HBM), luma and chroma sets at the same N; N = 4
with the DST on the luma set and the DCT on the chroma set, 16 and 32.  QP 32 on
the 8-bit stream at N = 4 / 16; QP 4 on the wide stream ((picture - 128) * 32 +
128) at N = 32, where an 8-bit source reconstructs to a constant.

Every repetition alternates, in this process, among six calls: the decoder at
N, the intra_rdo_closed_n call whose modes and levels it decodes, the N = 8
decoder / encoder pair (intra_decode_closed / intra_rdo_closed) on the 8-bit
stream at QP 32, and stage R alone at N and at 8 on the same levels.  Bar
(DESIGN.md §4.4c's for a decoder, not a correctness condition): decoder below
1x its encoder at every N.

Before timing, every decoder's output is compared with its encoder's
reconstruction over the whole stream (equal, or the tool stops).

HIP events on the launch stream, warm-up first, medians and ranges; one JSON
line per N appended to --out (default profiles/r11/bench_decode_n.jsonl).  The
block-step figure divides the decoder's time minus stage R's by its block steps:
per call the bw + 2 bh steps of its largest plane times the passes over the
resident workers, block rows / resident one-wave workgroups and at least one;
the resident counts are the
compiler's occupancy figures of the built kernels times 256 CUs (--resident
overrides them).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-hevc_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_rdo_closed_n import timed_round  # noqa: E402
from bench_rdo_n import W, H, synth_stream  # noqa: E402

# one-wave workgroups resident on 256 CUs: waves per SIMD x 4 SIMDs x 256 (N = 8: §4.3b)
RESIDENT = {4: 8192, 8: 8192, 16: 7168, 32: 4096}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="4,16,32")
    ap.add_argument("--resident", default="", help="N:workers,... overriding the resident worker counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "bench_decode_n.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_n needs an MI355X"
    from nano_hevc import gpu
    resident = dict(RESIDENT)
    for item in filter(None, a.resident.split(",")):
        k, v = item.split(":")
        resident[int(k)] = int(v)
    F = a.frames
    buf = synth_stream(F)
    wide = ((buf.to(torch.int32) - 128) * 32 + 128).to(torch.int16)
    sets = gpu.yuv420_plane_sets(F, W, H)
    dev = torch.cuda.get_device_name(0)

    def zeros(dtype):
        return torch.zeros(buf.shape, dtype=dtype, device="cuda")
    lvl, rec, dec = zeros(torch.int32), zeros(torch.int16), zeros(torch.int16)
    lvl8, rec8, dec8 = zeros(torch.int32), zeros(torch.int16), zeros(torch.int16)
    res = zeros(torch.int16)

    def pair(n):
        """(encode, decode, qp) at N; encode() leaves the mode maps in ``m``."""
        src, qp = (wide, 4) if n == 32 else (buf, 32)
        m = {}
        if n == 4:   # DST luma, DCT chroma
            def encode():
                m["y"] = gpu.intra_rdo_closed_n(src, sets[:1], 4, qp, True, lvl=lvl, rec=rec)[0]
                m["c"] = gpu.intra_rdo_closed_n(src, sets[1:], 4, qp, False, lvl=lvl, rec=rec)[0]

            def decode():
                gpu.intra_decode_closed_n(m["y"], lvl, sets[:1], 4, qp, True, rec=dec)
                gpu.intra_decode_closed_n(m["c"], lvl, sets[1:], 4, qp, False, rec=dec)
            return encode, decode, qp

        def encode():
            m["a"] = gpu.intra_rdo_closed_n(src, sets, n, qp, False, lvl=lvl, rec=rec)[0]

        def decode():
            gpu.intra_decode_closed_n(m["a"], lvl, sets, n, qp, False, rec=dec)
        return encode, decode, qp

    m8 = {}

    def encode8():
        m8["a"] = gpu.intra_rdo_closed(buf, sets, 32, lvl=lvl8, rec=rec8)[0]

    def decode8():
        gpu.intra_decode_closed(m8["a"], lvl8, sets, 32, rec=dec8)

    def steps(n):
        """(block rows, passes over the resident workers, block steps) of one decode at N: per call the
        passes over its rows, rows / resident workers and at least 1 (DESIGN.md §4.3b counts N = 8's 17,216
        rows on 8,192 waves as two), times the bw + 2 bh steps of its largest plane (N = 4: two calls)."""
        rows = passes = total = 0
        for call in ((sets[:1], sets[1:]) if n == 4 else (sets,)):
            r = sum((s.height // n if s.width >= n else 0) * s.planes_per_group * s.num_groups for s in call)
            p = max(1.0, r / resident[n])
            rows, passes = rows + r, passes + p
            total += p * max(s.width // n + 2 * (s.height // n) for s in call)
        return rows, round(passes, 3), total

    def stage_r(n):
        """Stage R alone on the levels of the pair at N (the decoder runs it before the wavefront)."""
        if n == 8:
            return lambda: gpu.dequant_inv8x8(lvl8, sets, 32, out=res)
        qp = 4 if n == 32 else 32
        if n == 4:
            def run():
                gpu.dequant_inv_n(lvl, sets[:1], 4, qp, True, out=res)
                gpu.dequant_inv_n(lvl, sets[1:], 4, qp, False, out=res)
            return run
        return lambda: gpu.dequant_inv_n(lvl, sets, n, qp, False, out=res)

    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        encode, decode, qp = pair(n)
        for e, d, r, o in ((encode, decode, rec, dec), (encode8, decode8, rec8, dec8)):
            o.fill_(-12345)
            e()
            d()
            torch.cuda.synchronize()
            assert torch.equal(o, r), f"N = {n}: a decoder's output differs from its encoder's reconstruction"
        td, te, td8, te8, tr, tr8 = timed_round([decode, encode, decode8, encode8, stage_r(n), stage_r(8)], a.reps,
                                                a.warmup)

        def med(t):
            return t[len(t) // 2]

        def step_us(t_dec, t_r, nsteps):   # the wavefront's share of the decoder's time per block step
            return round(1000 * (med(t_dec) - med(t_r)) / nsteps, 3)
        rows, passes, st = steps(n)
        rows8, passes8, st8 = steps(8)
        ratio, ratio8 = med(td) / med(te), med(td8) / med(te8)
        ln = {"tool": "bench_decode_n", "device": dev, "n": n, "qp": qp, "frames": F, "width": W, "height": H,
              "source": "wide" if n == 32 else "8-bit", "reps": a.reps, "warmup": a.warmup,
              "decode_ms_per_frame": round(med(td) / F, 5), "decode_min_max": [round(td[0] / F, 5), round(td[-1] / F, 5)],
              "encode_ms_per_frame": round(med(te) / F, 5), "encode_min_max": [round(te[0] / F, 5), round(te[-1] / F, 5)],
              "n8_decode_ms_per_frame": round(med(td8) / F, 5),
              "n8_decode_min_max": [round(td8[0] / F, 5), round(td8[-1] / F, 5)],
              "n8_encode_ms_per_frame": round(med(te8) / F, 5),
              "n8_encode_min_max": [round(te8[0] / F, 5), round(te8[-1] / F, 5)],
              "decode_over_encode": round(ratio, 3), "n8_decode_over_encode": round(ratio8, 3),
              "stage_r_ms_per_frame": round(med(tr) / F, 5), "n8_stage_r_ms_per_frame": round(med(tr8) / F, 5),
              "block_rows": rows, "resident_workers": resident[n], "passes": passes, "block_steps": round(st, 1),
              "us_per_block_step": step_us(td, tr, st),
              "n8_block_rows": rows8, "n8_resident_workers": resident[8], "n8_passes": passes8,
              "n8_block_steps": round(st8, 1), "n8_us_per_block_step": step_us(td8, tr8, st8),
              "rec_equal": True, "bar": "decode_over_encode < 1", "bar_met": bool(ratio < 1)}
        if n == 4:
            ln["transforms"] = "DST luma, DCT chroma"
            ln["calls_per_decode"] = 2
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
