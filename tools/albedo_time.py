#!/usr/bin/env python3
"""Device times of albedo demodulation on one GPU.

scene.checker_floor_scene() at SIZE^2 (default 1024), SPP = TARGET_SPP (4).  After WARMUP untimed
rounds, the median of REPEATS (default 25, at least 20) timings of
  demodulate_ms             rvcp_demodulate_async out of place, its own events (rvcp_albedo_wait)
  demodulate_in_place_ms    the same with the output on the input
  remodulate_store_ms       rvcp_remodulate_async with both outputs (linear + RGBA8), against
  remodulate_rgba_only_ms   the RGBA8 store alone, and
  tonemap_ms                the plain tone map of the same frame (the library's launcher, which
                            it exports, between events on the stream: one kernel per timing)
  render_svgf_ms[off|on]    rvcp_render_svgf, a synchronous call into host memory: host wall time
  render_denoised_ms[off|on]  rvcp_render_denoised likewise, with the switch off and on in one
                            run, alternating (each value is the median of its own REPEATS calls)
and, per kernel, the achieved bytes/s against its minimum traffic as a fraction of the 8 TB/s HBM
peak: the demodulation reads 12 B colour and the two words of a 32-B texel (every line of the
G-buffer: 32 B) and writes 12 B (56 B per pixel), the fused store reads 44 B and writes 16 B
(60 B; the plain tone map 12 + 4 = 16 B).  Prints one JSON line.

    timeout -k 10 300 python tools/albedo_time.py [--size 1024] [--repeats 25] [--warmup 5]

(one process, a few seconds; run it under a time limit like every step that uses the GPU)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rvcp_amd                 # noqa: E402
from rvcp_amd import abi        # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, the peak DESIGN.md §4.4 uses
TARGET_SPP = 4


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
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.rvcp_launch_tonemap.argtypes = [P, u32, P, P, P]
    L.rvcp_launch_tonemap.restype = ctypes.c_int
    sc = rvcp_amd.scene.checker_floor_scene()
    push = sc.push_constant(123.0)
    i32, f32 = torch.int32, torch.float32
    z = lambda k, dt=f32: torch.zeros(n * n * k, dtype=dt, device="cuda")     # noqa: E731
    d_rgba, d_lin, d_g, d_irr, d_out = z(1, i32), z(3), z(8, i32), z(3), z(3)
    d_gamma = torch.zeros(257, dtype=f32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.cuda.synchronize()
    med = statistics.median
    res = dict(size=n, repeats=a.repeats, warmup=a.warmup, spp=TARGET_SPP,
               device=torch.cuda.get_device_name(0), version=L.rvcp_version().decode(),
               scene="checker_floor_scene", faces=len(sc.mesh.faces))

    def rounds(f):
        for _ in range(a.warmup):
            f()
        return [f() for _ in range(a.repeats)]

    with rvcp_amd.RayTracer(spp=TARGET_SPP) as rt:
        rt.upload_scene(sc)
        rt.render_async(push, n, n, d_rgba.data_ptr(), d_lin.data_ptr(), stream=s)
        rt.wait()
        rt.render_gbuffer_async(push, n, n, d_g.data_ptr(), stream=s)
        torch.cuda.synchronize()

        def demod(out):
            def f():
                rt.demodulate_async(d_lin.data_ptr(), d_g.data_ptr(), n, n, out.data_ptr(), stream=s)
                return rt.albedo_wait()[0]
            return f
        res["demodulate_ms"] = med(rounds(demod(d_irr)))
        keep = d_lin.clone()
        res["demodulate_in_place_ms"] = med(rounds(demod(d_lin)))    # (divides again each round)
        d_lin.copy_(keep)
        torch.cuda.synchronize()

        def remod(lin, rgba):
            def f():
                rt.remodulate_async(d_irr.data_ptr(), d_g.data_ptr(), n, n,
                                    lin.data_ptr() if lin is not None else 0,
                                    rgba.data_ptr() if rgba is not None else 0, stream=s)
                return rt.albedo_wait()[1]
            return f
        res["remodulate_store_ms"] = med(rounds(remod(d_out, d_rgba)))
        res["remodulate_rgba_only_ms"] = med(rounds(remod(None, d_rgba)))

        # the plain tone map of the same frame under a threshold table of the same shape (the
        # kernel's time does not depend on the table's values: eight probes per channel)
        d_gamma.copy_(torch.linspace(0.0, 1.0, 257, device="cuda"))
        torch.cuda.synchronize()

        def tonemap():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if L.rvcp_launch_tonemap(d_out.data_ptr(), n * n, d_gamma.data_ptr(), d_rgba.data_ptr(), s) != 0:
                raise RuntimeError("kernel launch failed")
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        res["tonemap_ms"] = med(rounds(tonemap))

        # the chains with the switch off and on, alternating within one run
        def wall(f):
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3
        t = [200.0]

        def svgf():
            t[0] += 1.0
            rt.render_svgf(n, n, t[0])

        def denoised():
            t[0] += 1.0
            rt.render_denoised(n, n, t[0])
        for name, f in (("render_svgf_ms", svgf), ("render_denoised_ms", denoised)):
            got = {False: [], True: []}
            steps = {False: [], True: []}
            for k in range(a.warmup + a.repeats):
                for on in (False, True):
                    rt.demodulation = on
                    f()                                  # the first frame of a history, untimed
                    ms = wall(f)
                    if k >= a.warmup:
                        got[on].append(ms)
                        steps[on].append(rt.last_svgf_filter_ms + rt.last_svgf_accumulate_ms
                                         if f is svgf else rt.last_denoise_ms)
            res[name] = dict(off=med(got[False]), on=med(got[True]))
            res[name.replace("_ms", "_filter_steps_ms")] = dict(off=med(steps[False]), on=med(steps[True]))
        rt.demodulation = False
    res["fused_store_minus_tonemap_ms"] = res["remodulate_store_ms"] - res["tonemap_ms"]
    for key, ms, nbytes in (("demodulate", res["demodulate_ms"], 56.0),
                            ("remodulate_store", res["remodulate_store_ms"], 60.0),
                            ("tonemap", res["tonemap_ms"], 16.0)):
        bps = nbytes * n * n / (ms * 1e-3) if ms > 0 else None
        res[f"{key}_bytes_per_s"] = bps
        res[f"{key}_fraction_of_hbm_peak"] = bps / HBM_PEAK if bps else None
    print(json.dumps(res, allow_nan=False))


if __name__ == "__main__":
    main()
