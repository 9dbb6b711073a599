"""Temporal reprojection and accumulation, the part that needs no GPU: struct
layouts, the defaults, the camera projection against the oracle's sample_ray, and the numpy
restatement of the step (tests/temporal_ref.py) held to its exact properties, to the geometry
of a camera move across the Cornell box and to the quality gate."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
import oracle as O
import rvcp_amd
from rvcp_amd import abi
from conftest import ROOT, scene_arrays

HEADER = os.path.join(ROOT, "include", "rvcp.h")
f32 = np.float32

# the gcc offsetof harness of test_layout_abi.py, for the two new structs
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
#define S(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  S(rvcp_temporal_params_t); F(rvcp_temporal_params_t, alpha_min);
  F(rvcp_temporal_params_t, max_history); F(rvcp_temporal_params_t, sigma_plane);
  F(rvcp_temporal_params_t, normal_min);
  S(rvcp_temporal_view_t); F(rvcp_temporal_view_t, position); F(rvcp_temporal_view_t, k);
  F(rvcp_temporal_view_t, right); F(rvcp_temporal_view_t, _pad0); F(rvcp_temporal_view_t, down);
  F(rvcp_temporal_view_t, _pad1); F(rvcp_temporal_view_t, forward); F(rvcp_temporal_view_t, _pad2);
  printf("MAX_HISTORY %u\nDENOISE %u\nABI %u\n", RVCP_TEMPORAL_MAX_HISTORY, RVCP_TEMPORAL_DENOISE,
         RVCP_ABI_VERSION);
  return 0;
}
"""

NEW_SYMBOLS = ("rvcp_temporal_params_default", "rvcp_temporal_view_from_push",
               "rvcp_temporal_accumulate_async", "rvcp_temporal_wait", "rvcp_render_temporal",
               "rvcp_temporal_reset")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


def moved_scene(delta=(60.0, 20.0, 0.0)):
    """The Cornell box seen from the default camera moved by `delta` (same orientation)."""
    sc = rvcp_amd.Scene.default()
    sc.camera.position = (sc.camera.position + np.asarray(delta, dtype=f32)).astype(f32)
    return sc


# ---------------------------------------------------------------------------- layout, binding
def test_struct_layouts_match_header(c_layout):
    assert c_layout["rvcp_temporal_params_t"] == 16 and c_layout["rvcp_temporal_view_t"] == 64
    for cname, dts in (("rvcp_temporal_params_t", (abi.TEMPORAL_PARAMS_DTYPE, T.PARAMS_DTYPE)),
                       ("rvcp_temporal_view_t", (abi.TEMPORAL_VIEW_DTYPE, T.VIEW_DTYPE))):
        for dt in dts:
            assert dt.itemsize == c_layout[cname]
            for field in dt.names:
                assert dt.fields[field][1] == c_layout[f"{cname}.{field}"], (cname, field)
    assert c_layout["MAX_HISTORY"] == abi.TEMPORAL_MAX_HISTORY == 65535
    assert c_layout["DENOISE"] == abi.TEMPORAL_DENOISE == 1
    # only functions and structs were added: the ABI revision and the version string stay
    assert c_layout["ABI"] == abi.ABI_VERSION == 2
    assert abi.load().rvcp_version() == b"rvcp-mi355x 0.3.0 (gfx950, ABI 2)"


def test_library_exports_the_new_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW_SYMBOLS if f not in exported]
    L = abi.load()
    for f in NEW_SYMBOLS:
        assert f in abi.EXPORTED
        assert getattr(L, f).argtypes is not None, f
        assert getattr(L, f).restype is ctypes.c_int, f
    for name in ("temporal_accumulate_async", "temporal_wait", "temporal_reset", "render_temporal"):
        assert callable(getattr(rvcp_amd.RayTracer, name))


def test_defaults_need_no_gpu():
    L = abi.load()
    p = np.zeros((), dtype=abi.TEMPORAL_PARAMS_DTYPE)
    assert L.rvcp_temporal_params_default(abi.ptr(p)) == abi.RVCP_OK
    assert p["alpha_min"] == f32(0.05) and int(p["max_history"]) == 32
    assert p["sigma_plane"] == f32(0.1) == abi.make_denoise_params()["sigma_plane"]
    assert p["normal_min"] == f32(0.9)
    assert L.rvcp_temporal_params_default(None) == abi.RVCP_E_INVALID
    assert abi.make_temporal_params().tobytes() == p.tobytes() == T.params().tobytes()
    q = abi.make_temporal_params(alpha_min=0.0, max_history=7)
    assert q["alpha_min"] == 0 and int(q["max_history"]) == 7 and q["normal_min"] == p["normal_min"]


def test_new_entry_points_reject_null_arguments():
    L = abi.load()
    p = ctypes.c_void_p(1)
    E = abi.RVCP_E_INVALID
    assert L.rvcp_temporal_accumulate_async(None, None, p, p, None, None, None, 8, 8, None, p, p,
                                            None, None) == E
    assert L.rvcp_temporal_wait(None, None) == E
    assert L.rvcp_temporal_reset(None) == E
    assert L.rvcp_render_temporal(None, p, 8, 8, None, 0, None, p, None, None, None, None, None) == E
    push = np.ascontiguousarray(rvcp_amd.Scene.default().push_constant(0.0)).reshape(())
    v = np.zeros((), dtype=abi.TEMPORAL_VIEW_DTYPE)
    assert L.rvcp_temporal_view_from_push(None, 8, 8, abi.ptr(v)) == E
    assert L.rvcp_temporal_view_from_push(abi.ptr(push), 8, 8, None) == E
    assert L.rvcp_temporal_view_from_push(abi.ptr(push), 0, 8, abi.ptr(v)) == E
    assert L.rvcp_temporal_view_from_push(abi.ptr(push), 8, 0, abi.ptr(v)) == E
    push["camera"]["up"][..., :3] = push["camera"]["forward"]     # forward x up = 0
    assert L.rvcp_temporal_view_from_push(abi.ptr(push), 8, 8, abi.ptr(v)) == E


def test_run_headless_temporal_argument():
    """interactive.run_headless: without `temporal` nothing changes (tracer.render with three
    arguments, or render_denoised); with it every frame goes through tracer.render_temporal,
    `denoise` passed along."""
    from rvcp_amd import interactive

    class Stub:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("render", "render_denoised", "render_temporal"):
                raise AttributeError(name)

            def f(*a):
                self.calls.append((name, a))
                return np.zeros((4, 4, 4), np.uint8)
            return f

    sc = rvcp_amd.Scene.default()
    t = Stub()
    interactive.run_headless(t, sc, 2, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0 + i)
    assert t.calls == [("render", (4, 4, 3.0)), ("render", (4, 4, 4.0))]
    t, d = Stub(), abi.make_denoise_params(iterations=1)
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0, denoise=d)
    assert [c[0] for c in t.calls] == ["render_denoised"]
    t, p = Stub(), abi.make_temporal_params()
    interactive.run_headless(t, sc, 2, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0 + i, temporal=p)
    assert [c[0] for c in t.calls] == ["render_temporal"] * 2
    assert t.calls[1][1][:3] == (4, 4, 4.0) and t.calls[1][1][3] is p and t.calls[1][1][4] is None
    t = Stub()
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0, temporal=p,
                             denoise=d)
    assert t.calls[0][0] == "render_temporal" and t.calls[0][1][3] is p and t.calls[0][1][4] is d


# ---------------------------------------------------------------------------- the projection
def scenes():
    sc = rvcp_amd.Scene.default()
    return {False: sc, True: rvcp_amd.scene.rotated_scene(sc)}


@pytest.mark.parametrize("rotated", [False, True])
def test_view_from_push_within_one_ulp_of_float64(rotated):
    """Against temporal_ref.view_f64 (numpy float64, no shared code).  One float32 ulp of the
    value; a component of a unit vector is held to one ulp of 1 at the most (a float64 zero and a
    float64 1e-17 are the same direction)."""
    W, H = 37, 23
    push = scenes()[rotated].push_constant(0.0)
    v = abi.temporal_view(push, W, H)
    cam = push["camera"]
    pos, k, r, d, f = T.view_f64(cam["position"], cam["forward"], cam["up"], cam["vertical_fov"], H)
    assert np.array_equal(bits(v["position"]), bits(cam["position"][:3]))
    for name, want in (("k", np.array([k])), ("right", r), ("down", d), ("forward", f)):
        got = np.atleast_1d(v[name]).astype(np.float64)
        ulp = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
        assert np.all(np.abs(got - want) <= np.maximum(ulp, 0 if name == "k" else 2.0 ** -46)), name
    assert v["_pad0"] == 0 and v["_pad1"] == 0 and v["_pad2"] == 0
    assert abs(float(v["k"]) - H / (2 * np.tan(np.radians(20.0)))) < 1e-5 * H     # PI = 3.1415926
    # the numpy record built from the same float64 values agrees to the same ulp
    w = T.view_of_push(push, H)
    for name in ("k", "right", "down", "forward"):
        assert np.all(np.abs(bits(v[name]).astype(np.int64) - bits(w[name]).astype(np.int64)) <= 1) \
            or np.allclose(v[name], w[name], rtol=0, atol=2.0 ** -46)


@pytest.mark.parametrize("rotated", [False, True])
def test_self_projection(rotated):
    """Through the frame's own view every hit lands within 0.05 px of its own pixel centre
    (measured: 0.019), so the identity mapping and a reprojection through the own view start
    and continue the same histories."""
    W, H = 37, 23
    g = R.cornell_gbuffer(W, H, rotated)
    hit = g["face"] != R.MISS
    view = abi.temporal_view(scenes()[rotated].push_constant(0.0), W, H)
    fx, fy, z, ok = T.project(view, g["position"], W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    err = np.maximum(np.abs(fx.astype(np.float64) - xs), np.abs(fy.astype(np.float64) - ys))[hit]
    print(f"self-projection: max |pixel error| {err.max():.4f} px over {hit.sum()} hits")
    assert ok[hit].all() and (z[hit] > 0).all()
    assert err.max() <= 0.05
    # three frames from this camera, the history started by the first: the lengths (the minimum
    # over the accepted taps, plus one) agree everywhere, whichever way the taps are found
    rng = np.random.default_rng(1)
    p = T.params()
    acc_id, len_id = T.accumulate(rng.random((H, W, 3)).astype(f32), g, None, None, None, None, p)
    acc_re, len_re = acc_id, len_id
    assert np.array_equal(len_id, R.filterable(g).astype(np.uint32))
    for frame in (2, 3):
        c = rng.random((H, W, 3)).astype(f32)
        acc_id, len_id = T.accumulate(c, g, acc_id, g, len_id, None, p)
        acc_re, len_re = T.accumulate(c, g, acc_re, g, len_re, view, p)
        assert np.array_equal(len_id, len_re)
        assert np.array_equal(len_id, frame * R.filterable(g).astype(np.uint32))


# measured with this file at 37 x 23 (the maximum over the pixels with four accepted taps of
# |history - own position| / 555, any channel); the gate is twice that.  The footprint of a
# pixel on the nearest wall is 0.016 in these units, so a tap one pixel off would fail.
GEOMETRY_MEASURED = {(37, 23): 0.00848}


def test_geometry_of_a_camera_move():
    """Two frames of the Cornell box, the second from a camera moved by (60, 20, 0).  With
    colour = position / 555 as the history, a zero current frame, alpha_min = 0 and a long
    history, the output of a pixel whose four taps are accepted is the bilinear history value
    (times 1 - 1/65535): it must equal the pixel's own position / 555."""
    W, H = 37, 23
    prev_g = R.cornell_gbuffer(W, H)
    cur_g = R.cpu_gbuffer(moved_scene(), W, H)
    view = abi.temporal_view(rvcp_amd.Scene.default().push_constant(0.0), W, H)
    p = T.params(alpha_min=0.0, max_history=65535)
    prev_c = (prev_g["position"] / f32(555.0)).astype(f32)
    prev_len = np.full((H, W), 65535, dtype=np.uint32)
    out, length, nt = T.accumulate(np.zeros((H, W, 3), f32), cur_g, prev_c, prev_g, prev_len, view,
                                   p, want_taps=True)
    filt = R.filterable(cur_g)
    four, some, none = filt & (nt == 4), filt & (nt >= 1) & (nt <= 3), filt & (nt == 0)
    err = np.abs(out.astype(np.float64) - cur_g["position"].astype(np.float64) / 555.0)[four].max()
    print(f"geometry {W}x{H}: four taps {four.sum()}, one to three {some.sum()}, "
          f"reset {none.sum()}, max error {err:.5f}")
    assert four.sum() > filt.sum() // 2 and some.sum() >= 1 and none.sum() >= 1
    assert np.all(length[four] == 65535) and np.all(length[none] == 1)
    assert err <= 2.0 * GEOMETRY_MEASURED[(W, H)]


# ---------------------------------------------------------------------------- exact properties
PARAM_SETS = [T.params(max_history=1), T.params(alpha_min=0.0, max_history=40, normal_min=0.8,
                                                sigma_plane=0.25)]


@pytest.mark.parametrize("p", PARAM_SETS, ids=["max_history_1", "alpha_min_0"])
@pytest.mark.parametrize("identity", [False, True])
def test_exact_properties(p, identity):
    W, H = 45, 31
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed=3, identity=identity, p=p)
    v = None if identity else view
    out, length, nt = T.accumulate(c, g, pc, pg, pl, v, p, want_taps=True)
    filt = R.filterable(g)
    assert (~filt).any() and (filt & (nt == 0)).any() and (filt & (nt > 0)).any()
    # a non-filterable pixel passes through with length 0, a pixel without history returns c
    # bit for bit with length 1
    assert np.array_equal(bits(out[~filt]), bits(c[~filt])) and np.all(length[~filt] == 0)
    fresh = filt & (nt == 0)
    assert np.array_equal(bits(out[fresh]), bits(c[fresh])) and np.all(length[fresh] == 1)
    # the length never exceeds max_history, though the history's does
    assert length.max() <= int(p["max_history"]) < pl.max()
    assert np.all(length[filt] >= 1)
    # rejected and non-filterable history texels feed nothing
    hot = pc.copy()
    hot[~R.filterable(pg) | (pl == 0)] = 1.0e30
    out_hot, _ = T.accumulate(c, g, hot, pg, pl, v, p)
    assert np.array_equal(bits(out_hot), bits(out))
    # no history at all: every filterable pixel starts one
    out0, len0 = T.accumulate(c, g, None, None, None, v, p)
    assert np.array_equal(bits(out0), bits(c)) and np.array_equal(len0, filt.astype(np.uint32))


def test_identical_frames_come_back():
    """History == current (colour and G-buffer), identity mapping: h = c, so out = c + alpha * 0."""
    W, H = 37, 23
    g = R.cornell_gbuffer(W, H)
    rng = np.random.default_rng(2)
    c = rng.random((H, W, 3)).astype(f32)
    pl = rng.integers(1, 50, (H, W)).astype(np.uint32)
    p = T.params()
    out, length = T.accumulate(c, g, c, g, pl, None, p)
    assert np.array_equal(bits(out), bits(c))
    filt = R.filterable(g)
    assert np.array_equal(length[filt], np.minimum(pl[filt] + 1, 32))


# ---------------------------------------------------------------------------- quality
@pytest.mark.slow
def test_quality_gate_cornell_64_spp4_8_frames():
    W = H = 64
    sc = rvcp_amd.Scene.default()
    g = R.cornell_gbuffer(W, H)
    mask = R.filterable(g)
    ref = R.cornell_reference(W, H)
    p = abi.make_temporal_params()
    acc = length = None
    raw = []
    for t in T.QUALITY_SEEDS:
        noisy, _, _ = O.render(scene_arrays(sc), sc.push_constant(t), abi.make_config(spp=4), W, H)
        acc, length = T.accumulate(noisy, g, acc, None if acc is None else g, length, None, p)
        raw.append(R.rmse(noisy, ref, mask))
    first, before, after = raw[0], raw[-1], R.rmse(acc, ref, mask)
    print(f"rmse first raw {first:.4f} last raw {before:.4f} accumulated {after:.4f} "
          f"ratio to the first {after / first:.4f} gate {T.QUALITY_GATE:.4f}")
    assert np.all(length[mask] == 8) and np.all(length[~mask] == 0)
    assert 0.0 < T.QUALITY_GATE < 1.0
    assert after <= T.QUALITY_GATE * first
