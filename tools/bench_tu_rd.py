#!/usr/bin/env python3
"""Time of config 4's TU-size search and map-driven encode (gpu.tu_rd_planes,
gpu.tu_encode_map_planes) on one MI355X, next to the seeded
open-loop encoder on the same frames.

Workload: batches of 4K YUV420 frames (synthetic 8-bit content resident in HBM), the
luma set with CTB 32 and the DST, the U+V set with CTB 16 and without it.  Every
repetition alternates, in this process, among three calls:
  search   gpu.tu_rd_planes on both sets (every TU size per sample, the quadtree chosen);
  map      gpu.tu_encode_map_planes on both sets with the seeded encoder's maps;
  seeded   gpu.tu_pipeline_planes on both sets (the quadtree from the seed's hash).
Before timing, the map-driven levels and reconstruction are compared with the
seeded call's over the whole batch, and the search's sum J with the map-driven sum J
per plane (equal / not larger, or the tool stops).

HIP events on the launch stream, warm-up first, medians and ranges; one JSON line
per batch size appended to --out (default profiles/r12/bench_tu_rd.jsonl).
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

W, H = 3840, 2160
SEED = 1234


def synth_stream(gpu, frames, seed=5):
    """4K YUV420 frames back to back: waves + noise with flat and ramp regions, 8-bit, int16."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    fe = gpu.yuv420_frame_elems(W, H)
    buf = torch.empty(frames * fe, dtype=torch.int16, device="cuda")
    for f in range(frames):
        off = f * fe
        for (h, w) in ((H, W), (H // 2, W // 2), (H // 2, W // 2)):
            yy = torch.arange(h, device="cuda").view(h, 1).float()
            xx = torch.arange(w, device="cuda").view(1, w).float()
            a = 128 + 60 * torch.sin(xx / 5 + yy / 9 + f) + 40 * torch.cos(yy / 3 - xx / 11)
            a = a + torch.randint(-6, 7, (h, w), device="cuda", generator=g)
            a[:h // 3, :w // 2] = 90.0
            a[:h // 3, w // 2:] = (40 + 0.05 * xx + 0.03 * yy).expand(h, w)[:h // 3, w // 2:]
            buf[off:off + h * w] = a.clamp(0, 255).to(torch.int16).view(-1)
            off += h * w
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="16,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--lam", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "bench_tu_rd.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tu_rd needs an MI355X"
    from nano_hevc import gpu
    dev = torch.cuda.get_device_name(0)
    lines = []
    for F in [int(x) for x in a.frames.split(",")]:
        buf = synth_stream(gpu, F)
        sy, suv = gpu.yuv420_plane_sets(F, W, H)

        def zeros(dtype):
            return torch.zeros(buf.shape, dtype=dtype, device="cuda")
        lvl_s, rec_s, lvl_m, rec_m, lvl_r, rec_r = (zeros(torch.int32), zeros(torch.int16), zeros(torch.int32),
                                                   zeros(torch.int16), zeros(torch.int32), zeros(torch.int16))
        tuy = torch.zeros((F, H // 4, W // 4), dtype=torch.uint8, device="cuda")
        tuc = torch.zeros((2 * F, H // 8, W // 8), dtype=torch.uint8, device="cuda")
        tuy_r, tuc_r, pmy, pmc, pmy_m, pmc_m = (torch.zeros_like(tuy), torch.zeros_like(tuc), torch.zeros_like(tuy),
                                                torch.zeros_like(tuc), torch.zeros_like(tuy), torch.zeros_like(tuc))
        st = {}

        def seeded():
            gpu.tu_pipeline_planes(buf, sy, 32, 0, SEED, a.qp, True, lvl=lvl_s, rec=rec_s, tu=tuy)
            gpu.tu_pipeline_planes(buf, suv, 16, 1, SEED, a.qp, False, lvl=lvl_s, rec=rec_s, tu=tuc)

        def by_map():
            st["my"] = gpu.tu_encode_map_planes(buf, tuy, sy, 32, a.qp, a.lam, True, lvl=lvl_m, rec=rec_m, pm=pmy_m)[3]
            st["mc"] = gpu.tu_encode_map_planes(buf, tuc, suv, 16, a.qp, a.lam, False, lvl=lvl_m, rec=rec_m, pm=pmc_m)[3]

        def search():
            st["ry"] = gpu.tu_rd_planes(buf, sy, 32, a.qp, a.lam, True, lvl=lvl_r, rec=rec_r, tu=tuy_r, pm=pmy)[4]
            st["rc"] = gpu.tu_rd_planes(buf, suv, 16, a.qp, a.lam, False, lvl=lvl_r, rec=rec_r, tu=tuc_r, pm=pmc)[4]

        seeded()
        by_map()
        search()
        torch.cuda.synchronize()
        assert torch.equal(lvl_m, lvl_s) and torch.equal(rec_m, rec_s), "map-driven encode differs from the seeded call"
        assert bool((st["ry"][:, 0] <= st["my"][:, 0]).all()) and bool((st["rc"][:, 0] <= st["mc"][:, 0]).all()), \
            "the search's sum J exceeds the seeded map's"
        shares = [round(float((tuy_r == v).float().mean().item()), 4) for v in (2, 3, 4, 5)]
        ts, tm, tr = timed_round([search, by_map, seeded], a.reps, a.warmup)

        def med(t):
            return t[len(t) // 2]
        ln = {"tool": "bench_tu_rd", "device": dev, "frames": F, "width": W, "height": H, "qp": a.qp, "lambda": a.lam,
              "reps": a.reps, "warmup": a.warmup,
              "search_ms_per_frame": round(med(ts) / F, 5), "search_min_max": [round(ts[0] / F, 5), round(ts[-1] / F, 5)],
              "map_ms_per_frame": round(med(tm) / F, 5), "map_min_max": [round(tm[0] / F, 5), round(tm[-1] / F, 5)],
              "seeded_ms_per_frame": round(med(tr) / F, 5), "seeded_min_max": [round(tr[0] / F, 5), round(tr[-1] / F, 5)],
              "search_over_map": round(med(ts) / med(tm), 3), "map_over_seeded": round(med(tm) / med(tr), 3),
              "map_equals_seeded": True, "search_luma_area_shares_4_8_16_32": shares,
              "sum_j_search_over_seeded_map": round(float(st["ry"][:, 0].sum().item() + st["rc"][:, 0].sum().item()) /
                                                    float(st["my"][:, 0].sum().item() + st["mc"][:, 0].sum().item()), 4)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
        del buf, lvl_s, rec_s, lvl_m, rec_m, lvl_r, rec_r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
