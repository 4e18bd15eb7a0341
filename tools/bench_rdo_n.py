#!/usr/bin/env python3
"""Time of the NxN 35-mode open-loop RDO (gpu.intra_rdo_planes_n) on one MI355X.

Workload: a stream of --frames 1080p YUV420 frames (synthetic 8-bit content
resident in HBM) through intra_rdo_planes_n at N = 4 (DST on the luma set, DCT
on the chroma set), 16 and 32, and at N = 8 through the existing
intra_rdo_planes for scale.  QP 4 at N = 32 (every level is 0 from about QP 22
upward there), QP 22 otherwise.

Bar (N = 32 only): one luma plane through the new kernel against
tc32_plane(variant=0) -- the butterfly k_tu_process<32>, one chain per block where
the new kernel runs 35 -- on the same plane, the two calls alternating in this
process: t_rdo <= 1.2 * 35 * t_tc32.

HIP events on the launch stream, warm-up first, medians; one JSON line per N
appended to --out (default profiles/r09/bench_rdo_n.jsonl).  Registers, waves
per SIMD and LDS per workgroup come from the compiler's resource remarks for
csrc/nh_rdo_n.hip (--no-resources skips them).
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-hevc_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

W, H = 1920, 1080


def synth_stream(frames, seed=5):
    """YUV420 frames back to back: waves + noise, 8-bit, int16."""
    from nano_hevc import gpu
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
            buf[off:off + h * w] = a.clamp(0, 255).to(torch.int16).view(-1)
            off += h * w
    return buf


def timed_pair(fa, fb, reps, warmup):
    """Medians (ms) of fa and fb timed alternately (a, b, a, b, ...) in this process."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in evs:
        e[0].record(st)
        fa()
        e[1].record(st)
        fb()
        e[2].record(st)
    torch.cuda.synchronize()
    ta = sorted(e[0].elapsed_time(e[1]) for e in evs)
    tb = sorted(e[1].elapsed_time(e[2]) for e in evs)
    return ta[len(ta) // 2], tb[len(tb) // 2], (ta[0], ta[-1]), (tb[0], tb[-1])


def kernel_resources():
    """{N key: {vgprs, waves_per_simd, lds_bytes, scratch}} from -Rpass-analysis=kernel-resource-usage."""
    src = os.path.join(ROOT, "nano-hevc_amd", "csrc", "nh_rdo_n.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o",
                        os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out, cur = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*k_intra_rdo_nILi(\d+)ELb([01])E", ln)
        if m:
            cur = out.setdefault(f"{m.group(1)}{'dst' if m.group(2) == '1' else ''}", {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, ln)
            if m:
                cur[key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "bench_rdo_n.jsonl"))
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rdo_n needs an MI355X"
    from nano_hevc import gpu
    res = {} if a.no_resources else kernel_resources()
    F = a.frames
    buf = synth_stream(F)
    sets = gpu.yuv420_plane_sets(F, W, H)
    lvl = torch.zeros(buf.shape, dtype=torch.int32, device="cuda")
    rec = torch.zeros(buf.shape, dtype=torch.int16, device="cuda")
    dev = torch.cuda.get_device_name(0)

    def stream_n(n, qp):
        if n == 8:
            return lambda: gpu.intra_rdo_planes(buf, sets, qp, lvl=lvl, rec=rec)
        if n == 4:   # DST luma, DCT chroma
            def f():
                gpu.intra_rdo_planes_n(buf, sets[:1], 4, qp, True, lvl=lvl, rec=rec)
                gpu.intra_rdo_planes_n(buf, sets[1:], 4, qp, False, lvl=lvl, rec=rec)
            return f
        return lambda: gpu.intra_rdo_planes_n(buf, sets, n, qp, False, lvl=lvl, rec=rec)

    qps = {4: 22, 8: 22, 16: 22, 32: 4}
    f8 = stream_n(8, qps[8])
    lines = []
    for n in (4, 16, 32, 8):
        # every N alternates with the N = 8 stream, so the lines share one scale
        t, t8, sp, sp8 = timed_pair(stream_n(n, qps[n]), f8, a.reps, a.warmup)
        blocks = sum((s.width // n) * (s.height // n) * s.planes_per_group * s.num_groups for s in sets)
        ln = {"tool": "bench_rdo_n", "device": dev, "n": n, "qp": qps[n], "frames": F, "width": W, "height": H,
              "ms_per_frame": round(t / F, 5), "ms_per_frame_min_max": [round(x / F, 5) for x in sp],
              "n8_ms_per_frame_same_window": round(t8 / F, 5), "blocks_per_frame": blocks // F,
              "ns_per_block_mode": round(t * 1e6 / (blocks * 35), 3), "reps": a.reps, "warmup": a.warmup}
        if n == 4:
            ln["transforms"] = "DST luma, DCT chroma"
            ln["resources"] = {"dst": res.get("4dst"), "dct": res.get("4")}
        elif n != 8:
            ln["resources"] = res.get(str(n))
        if n == 32:
            y = buf[:W * H].view(H, W)
            yl = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            yr = torch.zeros((H, W), dtype=torch.int16, device="cuda")
            yset = [gpu.plane_set(0, W, H)]
            trdo, ttc, s1, s2 = timed_pair(lambda: gpu.intra_rdo_planes_n(buf, yset, 32, qps[32], False, lvl=lvl, rec=rec),
                                           lambda: gpu.tc32_plane(y, qps[32], 0, lvl=yl, rec=yr), a.reps, a.warmup)
            # the same 16 luma planes through both, per plane (tc32_planes variant 0: a launch per plane)
            ysets = sets[:1]
            srdo, stc, _, _ = timed_pair(lambda: gpu.intra_rdo_planes_n(buf, ysets, 32, qps[32], False, lvl=lvl, rec=rec),
                                         lambda: gpu.tc32_planes(buf, ysets, qps[32], 0, lvl=lvl, rec=rec), a.reps, a.warmup)
            ln["bar"] = {"luma_plane_ms": round(trdo, 5), "luma_plane_ms_min_max": [round(x, 5) for x in s1],
                         "tc32_variant0_plane_ms": round(ttc, 5), "tc32_variant0_ms_min_max": [round(x, 5) for x in s2],
                         "ratio_to_35x": round(trdo / (35 * ttc), 4), "limit": 1.2, "met": bool(trdo <= 1.2 * 35 * ttc),
                         "stream_luma_plane_ms": round(srdo / F, 5), "stream_tc32_variant0_plane_ms": round(stc / F, 5),
                         "stream_ratio_to_35x": round(srdo / (35 * stc), 4)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
