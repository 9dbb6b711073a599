#!/usr/bin/env python3
"""Device times of the SVGF steps on one GPU.

Cornell box at SIZE^2 (default 1024), SPP = TARGET_SPP (4), the previous frame from the default
camera and the current one from a camera moved by (60, 20, 0).  After WARMUP untimed rounds, the
median of REPEATS (default 25, at least 20) HIP-event timings of
  svgf_accumulate_ms        rvcp_svgf_accumulate_async through the previous view (four taps), its
                            own events (rvcp_svgf_wait), against temporal_reproject_ms:
                            rvcp_temporal_accumulate_async on the same buffers in the same run
  guided_pass_ms[i]         one variance-guided pass at step 2^i (the library's choice of kernel:
                            the LDS tile at steps 1 and 2, direct loads beyond), against
  plain_pass_ms[i]          the plain a-trous pass of §4.9 at the same step, and, for steps 1, 2,
  guided_direct_pass_ms[i]  the same guided pass through the direct kernel
                            (these three drive the library's kernel launchers, which it exports,
                            between events on the stream: one kernel per timing)
  variance_long_ms          the variance kernel on a frame whose histories are all spatial_below
                            long or longer (no workgroup stages anything) and
  variance_short_ms         on one whose histories are all of length 1 (every workgroup stages its
                            tile and every pixel takes the 7 x 7 estimate)
  svgf_filter_ms            rvcp_svgf_filter_async at the defaults on what the accumulation left,
                            variance output and RGBA8 store included (rvcp_svgf_wait)
  render_spp30_ms           the same run's plain frame at SPP = 30, rvcp_stats_t.kernel_ms
and, per kernel, the achieved bytes/s against its minimum traffic as a fraction of the 8 TB/s HBM
peak: a guided pass reads 12 B colour + 4 B variance + 32 B guide and writes 16 B per pixel (64 B),
the variance kernel reads 44 B and writes 4 B (48 B), the accumulation 124 B.  Prints one JSON line.

    timeout -k 10 300 python tools/svgf_time.py [--size 1024] [--repeats 25] [--warmup 5]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, the peak DESIGN.md §4.4 uses
TARGET_SPP = 4
MOVE = (60.0, 20.0, 0.0)
PASSES = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    import torch
    n = a.size
    L = abi.load()
    P, u32, f32c = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    L.rvcp_launch_svgf_variance.argtypes = [P, P, P, P, u32, u32, u32, u32, f32c, P]
    L.rvcp_launch_svgf_pass.argtypes = [P, P, P, P, P, u32, u32, u32, u32, u32, f32c, f32c, f32c, u32, P]
    L.rvcp_launch_denoise_pass.argtypes = [P, P, P, u32, u32, u32, u32, u32, f32c, f32c, P]
    for name in ("rvcp_launch_svgf_variance", "rvcp_launch_svgf_pass", "rvcp_launch_denoise_pass"):
        getattr(L, name).restype = ctypes.c_int
    sc = rvcp_amd.Scene.default()
    moved = rvcp_amd.Scene.default()
    moved.camera.position = (moved.camera.position + np.asarray(MOVE, np.float32)).astype(np.float32)
    push_prev, push_cur = sc.push_constant(123.0), moved.push_constant(124.0)
    i32, f32 = torch.int32, torch.float32
    z = lambda k, dt=f32: torch.zeros(n * n * k, dtype=dt, device="cuda")     # noqa: E731
    d_rgba = z(1, i32)
    d_lin, d_g = [z(3), z(3)], [z(8, i32), z(8, i32)]            # prev, cur
    d_len, d_mom = [z(1, i32), z(1, i32)], [z(2), z(2)]          # prev, out
    d_acc, d_out, d_var, d_tmp, d_vtmp = z(3), z(3), z(1), z(3), z(1)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()
    med = statistics.median
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, spp=TARGET_SPP,
               device=torch.cuda.get_device_name(0), version=L.rvcp_version().decode())
    sp = abi.make_svgf_params()
    res["params"] = {k: float(sp[k]) for k in sp.dtype.names if k != "_pad"}

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    def timed(launch):
        def f():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if launch() != 0:
                raise RuntimeError("kernel launch failed")
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        return med(rounds(f))

    with rvcp_amd.RayTracer(spp=30) as rt:
        rt.upload_scene(sc)

        def render30():
            rt.render_async(push_cur, n, n, d_rgba.data_ptr(), d_lin[1].data_ptr(), stream=s)
            return float(rt.wait()["kernel_ms"])
        res["render_spp30_ms"] = med(rounds(render30))

    with rvcp_amd.RayTracer(spp=TARGET_SPP) as rt:
        rt.upload_scene(sc)
        for k, push in ((0, push_prev), (1, push_cur)):
            rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin[k].data_ptr(), stream=s)
            rt.wait()
            rt.render_gbuffer_async(push, n, n, d_g[k].data_ptr(), stream=s)
        # the previous frame's history: every filterable pixel at length 1 with its own moments
        rt.svgf_accumulate_async(None, d_lin[0].data_ptr(), d_g[0].data_ptr(), 0, 0, 0, 0, n, n,
                                 d_acc.data_ptr(), d_len[0].data_ptr(), d_mom[0].data_ptr(), stream=s)
        rt.svgf_wait()
        d_lin[0].copy_(d_acc)
        torch.cuda.synchronize()
        view = abi.temporal_view(push_prev, n, n)

        def svgf_step():
            rt.svgf_accumulate_async(view, d_lin[1].data_ptr(), d_g[1].data_ptr(),
                                     d_lin[0].data_ptr(), d_g[0].data_ptr(), d_len[0].data_ptr(),
                                     d_mom[0].data_ptr(), n, n, d_acc.data_ptr(),
                                     d_len[1].data_ptr(), d_mom[1].data_ptr(), stream=s)
            return rt.svgf_wait()[0]

        def temporal_step():
            rt.temporal_accumulate_async(view, d_lin[1].data_ptr(), d_g[1].data_ptr(),
                                         d_lin[0].data_ptr(), d_g[0].data_ptr(),
                                         d_len[0].data_ptr(), n, n, d_out.data_ptr(),
                                         d_len[1].data_ptr(), stream=s)
            return rt.temporal_wait()
        res["temporal_reproject_ms"] = med(rounds(temporal_step))
        res["svgf_accumulate_ms"] = med(rounds(svgf_step))          # leaves d_acc, d_len[1], d_mom[1]
        res["reproject_continued"] = float((d_len[1] == 2).float().mean())

        def filt():
            rt.svgf_filter_async(d_acc.data_ptr(), d_mom[1].data_ptr(), d_len[1].data_ptr(),
                                 d_g[1].data_ptr(), n, n, d_out.data_ptr(), d_var.data_ptr(), 0,
                                 d_rgba.data_ptr(), sp, stream=s)
            return rt.svgf_wait()[1]
        res["svgf_filter_ms"] = med(rounds(filt))

        # single kernels through the library's launchers
        npl2, below = int(sp["normal_power_log2"]), int(sp["spatial_below"])
        sig_p, eps = float(sp["sigma_plane"]), float(sp["epsilon"])
        sl2 = float(np.float32(sp["sigma_luminance"]) * np.float32(sp["sigma_luminance"]))
        filterable = d_len[1] > 0

        def variance():
            return L.rvcp_launch_svgf_variance(d_mom[1].data_ptr(), d_len[1].data_ptr(),
                                               d_g[1].data_ptr(), d_var.data_ptr(), n, n, below,
                                               npl2, sig_p, s)
        keep = d_len[1].clone()
        d_len[1].copy_(filterable.to(i32) * below)
        torch.cuda.synchronize()
        res["variance_long_ms"] = timed(variance)
        d_len[1].copy_(filterable.to(i32))
        torch.cuda.synchronize()
        res["variance_short_ms"] = timed(variance)
        d_len[1].copy_(keep)
        torch.cuda.synchronize()
        variance()                                                   # the mixed frame's variance

        def guided(step, direct):
            return lambda: L.rvcp_launch_svgf_pass(
                d_acc.data_ptr(), d_var.data_ptr(), d_g[1].data_ptr(), d_tmp.data_ptr(),
                d_vtmp.data_ptr(), n, n, step, npl2, 1, sl2, eps, sig_p, 1 if direct else 0, s)

        def plain(step):
            return lambda: L.rvcp_launch_denoise_pass(d_acc.data_ptr(), d_g[1].data_ptr(),
                                                      d_tmp.data_ptr(), n, n, step, npl2, 0, 1.0,
                                                      sig_p, s)
        res["guided_pass_ms"] = [timed(guided(1 << i, False)) for i in range(PASSES)]
        res["plain_pass_ms"] = [timed(plain(1 << i)) for i in range(PASSES)]
        res["guided_direct_pass_ms"] = [timed(guided(1 << i, True)) for i in range(2)]
    res["svgf_step_ms"] = res["svgf_accumulate_ms"] + res["svgf_filter_ms"]
    res["cheaper_than_spp30_frame"] = res["svgf_step_ms"] < res["render_spp30_ms"]
    res["lds_beats_direct"] = [res["guided_pass_ms"][i] < res["guided_direct_pass_ms"][i]
                               for i in range(2)]
    for key, ms, nbytes in [("accumulate", res["svgf_accumulate_ms"], 124.0),
                            ("variance_long", res["variance_long_ms"], 48.0),
                            ("variance_short", res["variance_short_ms"], 48.0)] + \
                           [(f"guided_pass{i}", res["guided_pass_ms"][i], 64.0) for i in range(PASSES)]:
        bps = nbytes * n * n / (ms * 1e-3) if ms > 0 else None
        res[f"{key}_bytes_per_s"] = bps
        res[f"{key}_fraction_of_hbm_peak"] = bps / HBM_PEAK if bps else None
    print(json.dumps(res, allow_nan=False))


if __name__ == "__main__":
    main()
