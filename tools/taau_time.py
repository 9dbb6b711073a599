#!/usr/bin/env python3
"""Device times of the temporal upsampling step on one GPU.

Cornell box, output SIZE^2 (default 1024) from a frame traced at (SIZE / 2)^2, SPP = TARGET_SPP
(4).  After WARMUP untimed rounds, the median of REPEATS (default 25, at least 20) HIP-event
timings (rvcp_taau_wait) of rvcp_taa_upsample_async at scale 2
  taau_no_history_ms[_rgba]  without history: 3 B of traced colour read (12 B per traced pixel,
                             a quarter of the output pixels), 16 B written per output pixel
                             (+ 4 B RGBA8)
  taau_identity_ms[_rgba]    the camera at rest (one tap, q = p): + 16 B of history read
  taau_reproject_ms[_rgba]   through the views of a camera moved by (60, 20, 0) (four taps): + the
                             output-size texel's first 16 B
(the minimum traffic counts every byte once: the nine taps re-read the traced frame, the four
taps the history, out of the caches), each with the achieved bytes/s against that minimum as a
fraction of the 8 TB/s HBM peak;
  taau_direct_*_ms           the same step through the kernel's direct form (no LDS staging: nine
                             sample positions recomputed per lane), launched through the library's
                             internal launcher, without the RGBA8 store
and from the same run, as the yardstick,
  taa_reproject_ms / taa_reproject_rgba_ms   rvcp_taa_resolve_async at SIZE^2, reprojected
and, end to end on the host clock (render + G-buffer + steps + copies to the host) with the
camera at rest, rvcp_render_svgf and rvcp_render_temporal at SIZE^2 with TAA on at scale 1
against scale 2.  Prints one JSON line and, with --out, writes it to a file
(profiles/taau_time_1024sq.json is this tool's output).

    timeout -k 10 300 python tools/taau_time.py [--size 1024] [--repeats 25] [--warmup 5] [--out F]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import ctypes
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
SCALE = 2
MOVE = (60.0, 20.0, 0.0)
# per output pixel at scale 2, without RGBA8
MIN_BYTES = dict(no_history=12.0 / SCALE ** 2 + 16.0, identity=12.0 / SCALE ** 2 + 32.0,
                 reproject=12.0 / SCALE ** 2 + 48.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if a.size % SCALE:
        ap.error("--size must be even")
    import torch
    n, m = a.size, a.size // SCALE
    sc = rvcp_amd.Scene.default()
    moved = rvcp_amd.Scene.default()
    moved.camera.position = (moved.camera.position + np.asarray(MOVE, np.float32)).astype(np.float32)
    push_prev, push_cur = sc.push_constant(123.0), moved.push_constant(124.0)
    i32, f32 = torch.int32, torch.float32
    d_rgba = torch.zeros(n * n, dtype=i32, device="cuda")
    d_low = torch.zeros(m * m * 3, dtype=f32, device="cuda")        # the traced frame
    d_lin = torch.zeros(n * n * 3, dtype=f32, device="cuda")        # a full-size frame (yardstick)
    d_g = torch.zeros(n * n * 8, dtype=i32, device="cuda")          # the output-size G-buffer
    d_res = torch.zeros(n * n * 3, dtype=f32, device="cuda")        # the history
    d_wt = [torch.zeros(n * n, dtype=f32, device="cuda") for _ in range(2)]      # prev, out
    d_len = [torch.zeros(n * n, dtype=i32, device="cuda") for _ in range(2)]
    d_out = torch.zeros(n * n * 3, dtype=f32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    L = abi.load()
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.rvcp_launch_taa_upsample.argtypes = [P] * 8 + [u32] * 4 + [P] * 4 + [u32, P]
    L.rvcp_launch_taa_upsample.restype = ctypes.c_int
    med = statistics.median
    res = dict(size=n, traced=m, scale=SCALE, repeats=a.repeats, warmup=a.warmup, spp=TARGET_SPP,
               device=torch.cuda.get_device_name(0), version=abi.load().rvcp_version().decode())

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    with rvcp_amd.RayTracer(spp=TARGET_SPP) as rt:
        rt.upload_scene(sc)
        s = stream.cuda_stream
        # the history: frame 0 from the first camera, traced at m x m and upsampled without one
        jit_prev = rvcp_amd.taa_jitter_push(push_prev, m, m, rvcp_amd.taa_jitter(0))
        rt.render_async(jit_prev, m, m, d_rgba.data_ptr(), d_low.data_ptr(), stream=s)
        rt.wait()
        views = abi.temporal_view(push_cur, n, n), abi.temporal_view(push_prev, n, n)
        rt.taa_upsample_async(SCALE, abi.temporal_view(jit_prev, m, m), views[1], None,
                              d_low.data_ptr(), 0, 0, 0, n, n, d_res.data_ptr(),
                              d_wt[0].data_ptr(), stream=s)
        rt.taau_wait()
        # frame 1 through the jittered second camera at m x m, its G-buffer through the unjittered
        # one at n x n
        jit_cur = rvcp_amd.taa_jitter_push(push_cur, m, m, rvcp_amd.taa_jitter(1))
        jview = abi.temporal_view(jit_cur, m, m)
        rt.render_async(jit_cur, m, m, d_rgba.data_ptr(), d_low.data_ptr(), stream=s)
        rt.wait()
        rt.render_gbuffer_async(push_cur, n, n, d_g.data_ptr(), stream=s)

        def step(mode, rgba):
            hist = mode != "no_history"
            pv = views[1] if mode == "reproject" else None

            def f():
                rt.taa_upsample_async(SCALE, jview, views[0], pv, d_low.data_ptr(),
                                      d_g.data_ptr() if pv is not None else 0,
                                      d_res.data_ptr() if hist else 0,
                                      d_wt[0].data_ptr() if hist else 0, n, n, d_out.data_ptr(),
                                      d_wt[1].data_ptr(), d_rgba.data_ptr() if rgba else 0, stream=s)
                return rt.taau_wait()
            return med(rounds(f))
        tp = abi.make_taau_params()

        def direct(mode):
            hist = mode != "no_history"
            code = dict(no_history=0, identity=1, reproject=2)[mode]

            def f():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if L.rvcp_launch_taa_upsample(
                        d_low.data_ptr(), d_g.data_ptr(), d_res.data_ptr() if hist else None,
                        d_wt[0].data_ptr() if hist else None, d_out.data_ptr(), d_wt[1].data_ptr(),
                        None, None, n, n, SCALE, code, abi.ptr(jview), abi.ptr(views[0]),
                        abi.ptr(views[1]), abi.ptr(tp), 1, s) != 0:
                    raise RuntimeError("kernel launch failed")
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1)
            return med(rounds(f))
        for mode in ("no_history", "identity", "reproject"):
            res[f"taau_direct_{mode}_ms"] = direct(mode)
            res[f"taau_{mode}_ms"] = step(mode, False)
            if mode != "no_history":
                res[f"{mode}_continued"] = float((d_wt[1] > 0.15).float().mean())
            res[f"taau_{mode}_rgba_ms"] = step(mode, True)

        # the yardstick: the TAA resolve at n x n in the same run (history: a resolved frame 0)
        jit_full = rvcp_amd.taa_jitter_push(push_cur, n, n, rvcp_amd.taa_jitter(1))
        rt.render_async(push_prev, n, n, d_rgba.data_ptr(), d_lin.data_ptr(), stream=s)
        rt.wait()
        rt.render_gbuffer_async(push_prev, n, n, d_g.data_ptr(), stream=s)
        rt.taa_resolve_async(None, None, d_lin.data_ptr(), d_g.data_ptr(), 0, 0, n, n,
                             d_res.data_ptr(), d_len[0].data_ptr(), stream=s)
        rt.taa_wait()
        rt.render_async(jit_full, n, n, d_rgba.data_ptr(), d_lin.data_ptr(), stream=s)
        rt.wait()
        rt.render_gbuffer_async(jit_full, n, n, d_g.data_ptr(), stream=s)

        def resolve(rgba):
            def f():
                rt.taa_resolve_async(views[0], views[1], d_lin.data_ptr(), d_g.data_ptr(),
                                     d_res.data_ptr(), d_len[0].data_ptr(), n, n, d_out.data_ptr(),
                                     d_len[1].data_ptr(), d_rgba.data_ptr() if rgba else 0, stream=s)
                return rt.taa_wait()
            return med(rounds(f))
        res["taa_reproject_ms"] = resolve(False)
        res["taa_reproject_rgba_ms"] = resolve(True)

        # end to end, host clock around the synchronous calls, the camera at rest
        def wall(f):
            def g():
                t0 = time.perf_counter()
                f()
                return (time.perf_counter() - t0) * 1e3
            return med(rounds(g))
        seeds = iter(range(10 ** 6))
        rt.taa = True
        for scale in (1, SCALE):
            rt.taa_upsample = scale
            res[f"e2e_render_svgf_scale_{scale}_ms"] = wall(
                lambda: rt.render_svgf(n, n, float(next(seeds) % 1000)))
            res[f"e2e_render_svgf_scale_{scale}_path_kernel_ms"] = float(rt.last_stats["kernel_ms"])
            res[f"e2e_render_temporal_scale_{scale}_ms"] = wall(
                lambda: rt.render_temporal(n, n, float(next(seeds) % 1000)))
        rt.taa_upsample = 1
        rt.taa = False
    for mode, nbytes in MIN_BYTES.items():
        for suffix, extra in (("", 0.0), ("_rgba", 4.0)):
            ms = res[f"taau_{mode}{suffix}_ms"]
            key = f"{mode}{suffix}"
            res[f"{key}_min_bytes"] = (nbytes + extra) * n * n
            res[f"{key}_bytes_per_s"] = (nbytes + extra) * n * n / (ms * 1e-3) if ms > 0 else None
            res[f"{key}_fraction_of_hbm_peak"] = (res[f"{key}_bytes_per_s"] / HBM_PEAK
                                                  if res[f"{key}_bytes_per_s"] else None)
    res["fused_store_ms"] = res["taau_reproject_rgba_ms"] - res["taau_reproject_ms"]
    res["lds_beats_direct"] = {m: res[f"taau_{m}_ms"] < res[f"taau_direct_{m}_ms"]
                               for m in ("no_history", "identity", "reproject")}
    res["upsample_vs_resolve"] = res["taau_reproject_rgba_ms"] / res["taa_reproject_rgba_ms"]
    res["e2e_svgf_scale_2_vs_1"] = (res[f"e2e_render_svgf_scale_{SCALE}_ms"] /
                                    res["e2e_render_svgf_scale_1_ms"])
    res["e2e_temporal_scale_2_vs_1"] = (res[f"e2e_render_temporal_scale_{SCALE}_ms"] /
                                        res["e2e_render_temporal_scale_1_ms"])
    line = json.dumps(res, allow_nan=False)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
