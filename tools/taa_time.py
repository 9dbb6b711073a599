#!/usr/bin/env python3
"""Device times of the temporal anti-aliasing resolve on one GPU.

Cornell box at SIZE^2 (default 1024), SPP = TARGET_SPP (4).  After WARMUP untimed rounds, the
median of REPEATS (default 25, at least 20) HIP-event timings (rvcp_taa_wait) of
rvcp_taa_resolve_async
  taa_no_history_ms[_rgba]  without history: 12 B read, 16 B written per pixel (+ 4 B RGBA8)
  taa_identity_ms[_rgba]    the camera at rest (one tap, q = p): 28 B read, 16 B written
  taa_reproject_ms[_rgba]   through the views of a camera moved by (60, 20, 0) (four taps): 44 B
                            read -- 12 B colour, the texel's first 16 B, 16 B of history --, 16 B
                            written
(the minimum traffic counts every byte once: the 3 x 3 box re-reads the current frame, the four
taps re-read the history, out of the caches), each with the achieved bytes/s against that minimum
as a fraction of the 8 TB/s HBM peak, and from the same run, as yardsticks,
  temporal_reproject_ms / temporal_rgba_ms   rvcp_temporal_accumulate_async reprojected, without
                            and with its RGBA8 store (108 B per pixel, tools/temporal_time.py)
  tonemap_launch_ms         their difference: the plain tone-map launch the fused store replaces
and, end to end on the host clock (render + G-buffer + steps + copies to the host),
rvcp_render_svgf and rvcp_render_temporal with the switch off and on.  Prints one JSON line and,
with --out, writes it to a file (profiles/taa_time_1024sq.json is this tool's output).

    timeout -k 10 300 python tools/taa_time.py [--size 1024] [--repeats 25] [--warmup 5] [--out F]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, the peak DESIGN.md §4.4 uses
TARGET_SPP = 4
MOVE = (60.0, 20.0, 0.0)
MIN_BYTES = dict(no_history=28.0, identity=44.0, reproject=60.0)       # per pixel, without RGBA8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    import torch
    n = a.size
    sc = rvcp_amd.Scene.default()
    moved = rvcp_amd.Scene.default()
    moved.camera.position = (moved.camera.position + np.asarray(MOVE, np.float32)).astype(np.float32)
    push_prev, push_cur = sc.push_constant(123.0), moved.push_constant(124.0)
    i32, f32 = torch.int32, torch.float32
    d_rgba = torch.zeros(n * n, dtype=i32, device="cuda")
    d_lin = [torch.zeros(n * n * 3, dtype=f32, device="cuda") for _ in range(2)]     # prev, cur
    d_g = [torch.zeros(n * n * 8, dtype=i32, device="cuda") for _ in range(2)]
    d_len = [torch.zeros(n * n, dtype=i32, device="cuda") for _ in range(2)]         # prev, out
    d_res = torch.zeros(n * n * 3, dtype=f32, device="cuda")                         # TAA history
    d_out = torch.zeros(n * n * 3, dtype=f32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    med = statistics.median
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, spp=TARGET_SPP,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode())

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    with rvcp_amd.RayTracer(spp=TARGET_SPP) as rt:
        rt.upload_scene(sc)
        s = stream.cuda_stream
        # frame 0 (the history) from the first camera, frame 1 through the jittered second one
        jit_cur = rvcp_amd.taa_jitter_push(push_cur, n, n, rvcp_amd.taa_jitter(1))
        for push, k in ((push_prev, 0), (jit_cur, 1)):
            rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin[k].data_ptr(), stream=s)
            rt.wait()
            rt.render_gbuffer_async(push, n, n, d_g[k].data_ptr(), stream=s)
        # the histories: the resolved frame 0 (every pixel at length 1), and the temporal step's
        rt.taa_resolve_async(None, None, d_lin[0].data_ptr(), d_g[0].data_ptr(), 0, 0, n, n,
                             d_res.data_ptr(), d_len[0].data_ptr(), stream=s)
        rt.taa_wait()
        views = abi.temporal_view(push_cur, n, n), abi.temporal_view(push_prev, n, n)

        def resolve(mode, rgba):
            cv, pv = views if mode == "reproject" else (None, None)
            hist = mode != "no_history"

            def f():
                rt.taa_resolve_async(cv, pv, d_lin[1].data_ptr(), d_g[1].data_ptr(),
                                     d_res.data_ptr() if hist else 0,
                                     d_len[0].data_ptr() if hist else 0, n, n, d_out.data_ptr(),
                                     d_len[1].data_ptr(), d_rgba.data_ptr() if rgba else 0, stream=s)
                return rt.taa_wait()
            return med(rounds(f))
        for mode in ("no_history", "identity", "reproject"):
            res[f"taa_{mode}_ms"] = resolve(mode, False)
            if mode != "no_history":
                res[f"{mode}_continued"] = float((d_len[1] == 2).float().mean())
            res[f"taa_{mode}_rgba_ms"] = resolve(mode, True)

        # the yardstick: the temporal step of the same frames
        rt.temporal_accumulate_async(None, d_lin[0].data_ptr(), d_g[0].data_ptr(), 0, 0, 0, n, n,
                                     d_out.data_ptr(), d_len[0].data_ptr(), stream=s)
        rt.temporal_wait()
        d_lin[0].copy_(d_out)
        torch.cuda.synchronize()

        def temporal(rgba):
            def f():
                rt.temporal_accumulate_async(
                    views[1], d_lin[1].data_ptr(), d_g[1].data_ptr(), d_lin[0].data_ptr(),
                    d_g[0].data_ptr(), d_len[0].data_ptr(), n, n, d_out.data_ptr(),
                    d_len[1].data_ptr(), d_rgba.data_ptr() if rgba else 0, stream=s)
                return rt.temporal_wait()
            return med(rounds(f))
        res["temporal_reproject_ms"] = temporal(False)
        res["temporal_rgba_ms"] = temporal(True)
        res["tonemap_launch_ms"] = res["temporal_rgba_ms"] - res["temporal_reproject_ms"]

        # end to end, host clock around the synchronous calls, the camera at rest
        def wall(f):
            def g():
                t0 = time.perf_counter()
                f()
                return (time.perf_counter() - t0) * 1e3
            return med(rounds(g))
        seeds = iter(range(10 ** 6))
        for on in (False, True):
            rt.taa = on
            tag = "on" if on else "off"
            res[f"e2e_render_svgf_taa_{tag}_ms"] = wall(
                lambda: rt.render_svgf(n, n, float(next(seeds) % 1000)))
            res[f"e2e_render_temporal_taa_{tag}_ms"] = wall(
                lambda: rt.render_temporal(n, n, float(next(seeds) % 1000)))
        rt.taa = False
    for mode, nbytes in MIN_BYTES.items():
        for suffix, extra in (("", 0.0), ("_rgba", 4.0)):
            ms = res[f"taa_{mode}{suffix}_ms"]
            key = f"{mode}{suffix}"
            res[f"{key}_min_bytes"] = (nbytes + extra) * n * n
            res[f"{key}_bytes_per_s"] = (nbytes + extra) * n * n / (ms * 1e-3) if ms > 0 else None
            res[f"{key}_fraction_of_hbm_peak"] = (res[f"{key}_bytes_per_s"] / HBM_PEAK
                                                  if res[f"{key}_bytes_per_s"] else None)
    res["fused_store_ms"] = res["taa_reproject_rgba_ms"] - res["taa_reproject_ms"]
    res["resolve_vs_temporal"] = res["taa_reproject_rgba_ms"] / res["temporal_rgba_ms"]
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
