"""Temporal upsampling without a GPU: the C-ABI additions (layout, symbols,
defaults, NULL rejection -- every other RVCP_E_INVALID case needs a context, hence a device, and
lives in test_gpu_taau), exact properties of the float32 restatement of the step
(tests/taau_ref.py), the ghosting check and the flat-shade gate on CPU G-buffers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
import taa_ref as A
import taau_ref as U
import rvcp_amd
from rvcp_amd import abi
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rvcp.h")
f32 = np.float32
SEED = 5            # a seed at which the generators hold their mixes at every size used here

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
#define S(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  S(rvcp_taau_params_t); F(rvcp_taau_params_t, max_weight); F(rvcp_taau_params_t, init_weight);
  F(rvcp_taau_params_t, clamp); F(rvcp_taau_params_t, _pad);
  printf("PERIOD %u\nABI %u\n", RVCP_TAA_JITTER_PERIOD, RVCP_ABI_VERSION);
  return 0;
}
"""

NEW_SYMBOLS = ("rvcp_taau_params_default", "rvcp_taa_upsample_async", "rvcp_taau_wait",
               "rvcp_set_taa_upsample", "rvcp_get_taa_upsample")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("taau_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


# ---------------------------------------------------------------------------- layout, binding
def test_struct_layout_matches_header(c_layout):
    assert c_layout["rvcp_taau_params_t"] == 16
    for dt in (abi.TAAU_PARAMS_DTYPE, U.PARAMS_DTYPE):
        assert dt.itemsize == 16
        for field in dt.names:
            assert dt.fields[field][1] == c_layout[f"rvcp_taau_params_t.{field}"], field
    # the jitter period stays, and only functions, constants and one struct were added
    assert c_layout["PERIOD"] == abi.TAA_JITTER_PERIOD == 16
    assert c_layout["ABI"] == abi.ABI_VERSION == 2


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
    for name in ("taa_upsample_async", "taau_wait"):
        assert callable(getattr(rvcp_amd.RayTracer, name))
    assert isinstance(rvcp_amd.RayTracer.taa_upsample, property)


def test_defaults_need_no_gpu():
    L = abi.load()
    p = np.zeros((), dtype=abi.TAAU_PARAMS_DTYPE)
    p["_pad"] = 7
    assert L.rvcp_taau_params_default(abi.ptr(p)) == abi.RVCP_OK
    assert p["max_weight"] == f32(8.0) and p["init_weight"] == f32(0.1)
    assert int(p["clamp"]) == 1 and int(p["_pad"]) == 0
    assert L.rvcp_taau_params_default(None) == abi.RVCP_E_INVALID
    assert abi.make_taau_params().tobytes() == p.tobytes() == U.params().tobytes()
    q = abi.make_taau_params(max_weight=2.0, clamp=0)
    assert q["max_weight"] == 2 and int(q["clamp"]) == 0 and q["init_weight"] == f32(0.1)


def test_new_entry_points_reject_a_null_context():
    L = abi.load()
    p = ctypes.c_void_p(1)
    E = abi.RVCP_E_INVALID
    v = np.zeros((), dtype=abi.TEMPORAL_VIEW_DTYPE)
    assert L.rvcp_taa_upsample_async(None, 2, abi.ptr(v), abi.ptr(v), None, p, None, None, None,
                                     8, 8, None, p, p, None, None) == E
    assert L.rvcp_taau_wait(None, None) == E
    assert L.rvcp_set_taa_upsample(None, 2) == E
    assert L.rvcp_get_taa_upsample(None, p) == E


# ---------------------------------------------------------------------------- the restatement
MIX_SIZES = [(66, 46, 2), (130, 4, 2), (69, 45, 3), (12, 8, 4), (8, 8, 2), (64, 64, 4), (32, 16, 2)]


def test_generator_meets_its_mix():
    for W, H, s in MIX_SIZES:
        U.synthetic_case(W, H, s, SEED)         # asserts inside


def _bilinear_f64(c, s):
    """Bilinear upscaling by s with replicated borders, float64: output pixel centre
    (x + 1/2) / s - 1/2 in traced pixel coordinates."""
    h, w = c.shape[:2]
    c = np.asarray(c, dtype=np.float64)
    xs = np.clip((np.arange(w * s) + 0.5) / s - 0.5, 0, w - 1)
    ys = np.clip((np.arange(h * s) + 0.5) / s - 0.5, 0, h - 1)
    x0, y0 = np.minimum(np.floor(xs).astype(int), max(w - 2, 0)), np.minimum(np.floor(ys).astype(int), max(h - 2, 0))
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = (xs - x0)[None, :, None], (ys - y0)[:, None, None]
    top = c[y0][:, x0] * (1 - tx) + c[y0][:, x1] * tx
    bot = c[y1][:, x0] * (1 - tx) + c[y1][:, x1] * tx
    return top * (1 - ty) + bot * ty


@pytest.mark.parametrize("w,h,s", [(20, 14, 2), (23, 15, 3), (16, 16, 4), (1, 1, 2), (5, 1, 4)])
def test_zero_jitter_without_history_is_the_bilinear_reconstruction(w, h, s):
    """With the traced camera the output camera itself the samples lie on the regular grid
    s lx + (s - 1) / 2 and the wide tent's normalised sum is the bilinear interpolation
    (replicated at the border: the missing taps' weight is divided out).  Tolerance: a sample
    position carries a few roundings at the magnitude of W / 2 <= 32 (about 2^-18 pixels), so a
    tent weight is off by 2^-18 and a colour in [0, 1] summed over at most nine taps by less than
    1e-4."""
    rng = np.random.default_rng(3)
    c = rng.random((h, w, 3)).astype(f32)
    push = np.ascontiguousarray(rvcp_amd.Scene.default().push_constant(0.0)).reshape(())
    out, wt = U.upsample(c, s, T.view_of_push(push, h), T.view_of_push(push, h * s), None, None,
                         None, None, U.params())
    assert np.array_equal(bits(out), bits(U.wide_tent(c, s, push)))
    assert np.max(np.abs(out.astype(np.float64) - _bilinear_f64(c, s))) < 1e-4
    assert np.all(wt == U.params()["init_weight"])


PARAM_SETS = [U.params(), U.params(clamp=0), U.params(max_weight=0.1, init_weight=0.1)]


@pytest.mark.parametrize("p", PARAM_SETS, ids=["defaults", "clamp_0", "max_weight_is_init_weight"])
@pytest.mark.parametrize("mode", ["reprojection", "identity", "no_history"])
@pytest.mark.parametrize("W,H,s", [(66, 46, 2), (69, 45, 3), (64, 64, 4)])
def test_exact_properties(W, H, s, mode, p):
    """out lies within [0, 1] exactly when the history does: floating-point addition and
    multiplication by a non-negative number are monotone, so Sn <= Wn, h Wh <= Wh and the
    numerator <= Wt term by term, and likewise the history's and the wide tent's sums.

    A clamped pixel lies within its box up to a relative 2^-19: in exact arithmetic out is a
    convex combination of h (inside the box after the clamp) and of tap colours (the box is
    their hull).  All terms are non-negative, so relative errors only add up: Sn carries one
    rounding per product and at most nine per sum, Wn nine, h Wh one, the numerator's sum one, Wt
    one, the division one -- at most 22 roundings between the exact combination and out, and
    (1 + 2^-24)^22 - 1 < 2^-19."""
    c, jv, cv, pv, g, pr, pw = U.synthetic_case(W, H, s, SEED, p)
    if mode == "identity":
        pv = None
    if mode == "no_history":
        pr = pw = pv = None
    out, wt, info = U.upsample(c, s, jv, cv, pv, g, pr, pw, p, True)
    has = info["has"]
    assert out.dtype == f32 and wt.dtype == f32 and out.shape == (H, W, 3)
    assert not np.isnan(out).any() and out.min() >= 0.0 and out.max() <= 1.0
    # the weight never exceeds max_weight, and a history starts at init_weight
    assert np.all(wt <= p["max_weight"]) and np.all(wt > 0)
    assert np.all(wt[~has] == p["init_weight"])
    assert np.array_equal(bits(out[~has]), bits(info["cur"][~has]))
    if mode == "no_history":
        assert not has.any()
        return
    assert has.any() and (~has).any()
    if p["max_weight"] > 1:
        assert (wt[has] == p["max_weight"]).any() and (wt[has] < p["max_weight"]).any()
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    eps = 2.0 ** -19
    inside = np.all((out >= lo * (1 - eps)) & (out <= hi * (1 + eps)), axis=-1)
    ch = info["clamped"] & has
    # low-res border pixels are never clamped
    assert not info["clamped"][~info["interior"]].any() and not info["changed"][~info["interior"]].any()
    if int(p["clamp"]) == 1:
        assert ch.any() and np.all(inside[ch])
        assert info["changed"].any()
        free, _, finfo = U.upsample(c, s, jv, cv, pv, g, pr, pw, U.params(clamp=0), True)
        border = has & ~info["interior"]
        assert border.any()
        assert np.array_equal(bits(info["h"][border]), bits(finfo["h"][border]))
        outside = np.any((finfo["h"] < info["lo"] - 1e-3) | (finfo["h"] > info["hi"] + 1e-3), axis=-1)
        assert outside[border].any()           # ... though some of them lie outside their box
    else:
        assert not ch.any() and not info["changed"].any()
        assert not np.all(inside[info["interior"] & has])


# ---------------------------------------------------------------------------- ghosting
def test_ghosting_check():
    """The history is one constant colour absent from the frame, the camera moves by
    (60, 20, 0): one step with the clamp leaves every clamped pixel inside its box (up to the
    rounding bound of test_exact_properties), without it the ghost keeps Wh / (Wh + Wn) of its
    weight."""
    w, h, s = 20, 14, 2
    W, H = w * s, h * s
    sc = rvcp_amd.Scene.default()
    mats = sc.aligned_materials()
    g_hi = R.cornell_gbuffer(W, H)
    ghost = np.empty((H, W, 3), dtype=f32)
    ghost[...] = (0.05, 0.9, 0.45)
    wts = np.full((H, W), 4.0, dtype=f32)
    prev_push = np.ascontiguousarray(sc.push_constant(0.0)).reshape(())
    cur_push = prev_push.copy()
    cur_push["camera"]["position"][:3] += np.array([60.0, 20.0, 0.0], dtype=f32)
    # frame 2 of the jitter sequence: (1/4, 1/9 - 1/2) traced pixels puts the samples on the odd
    # output columns near the frame's centre, so the even ones have none under the narrow tent
    jp = A.jittered_push(prev_push, h, 2)
    c = A.flat_shade(A.cpu_gbuffer_of(jp, w, h), mats)
    jcur = jp.copy()
    jcur["camera"]["position"][:3] = cur_push["camera"]["position"][:3]
    jv = T.view_of_push(jcur, h)
    cv, pv = T.view_of_push(cur_push, H), T.view_of_push(prev_push, H)
    assert not np.any(np.all(np.isclose(A.sat(c), ghost[0, 0], atol=0.02), axis=-1))
    on, _, info = U.upsample(c, s, jv, cv, pv, g_hi, ghost, wts, U.params(clamp=1), True)
    off, _, oinfo = U.upsample(c, s, jv, cv, pv, g_hi, ghost, wts, U.params(clamp=0), True)
    m = info["clamped"] & info["has"]
    assert m.sum() > 0.5 * W * H
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    eps = 2.0 ** -19
    inside = lambda o: np.all((o >= lo * (1 - eps)) & (o <= hi * (1 + eps)), axis=-1)  # noqa: E731
    assert np.all(inside(on)[m])
    assert not np.all(inside(off)[m])
    assert not np.array_equal(bits(on), bits(off))
    # unclamped: the ghost's share is Wh / (Wh + Wn), the rest is the narrow sum
    Wh, Wn = oinfo["Wh"].astype(np.float64), oinfo["Wn"].astype(np.float64)
    assert np.allclose(Wh[m], 4.0, atol=1e-5)
    flat = m & np.all(info["hi"] - info["lo"] < 1e-6, axis=-1) & (Wn > 0)
    assert flat.any()
    share = (Wh / (Wh + Wn))[flat][:, None]
    assert np.allclose(off[flat], ghost[flat] * share + info["lo"][flat] * (1 - share), atol=1e-5)
    assert np.allclose(on[flat], info["lo"][flat], atol=1e-5)
    # no sample nearby: the unclamped ghost stays whole
    none = m & (Wn < 1e-4)
    assert none.sum() >= 8 and np.allclose(off[none], ghost[none], atol=1e-4)


# ---------------------------------------------------------------------------- the gate
@pytest.mark.slow
def test_flat_shade_gate_cornell_20x14_to_40x28():
    """16 jittered 20 x 14 frames of the flat-shaded Cornell box upsampled to 40 x 28 at the
    defaults, against the 4 x 4 supersampled 40 x 28 frame: the RMSE over the edge pixels and
    over all pixels must fall to RATIO_MEASURED plus a quarter of the distance to 1 of the
    bilinearly upscaled centred 20 x 14 frame's (comparator A), and the edge RMSE must lie below
    that of one centred 40 x 28 frame (comparator B), which costs four times the rays."""
    sc = rvcp_amd.Scene.default()
    r = U.flat_gate(20, 14, np.ascontiguousarray(sc.push_constant(0.0)).reshape(()),
                    sc.aligned_materials(), A.cpu_gbuffer_of)
    print("\nTAAU flat-shade gate 20x14 -> 40x28 (CPU G-buffers):", r)
    assert r["n_edge"] >= 100
    assert r["ratio_edge"] <= A.gate(U.RATIO_MEASURED["ratio_edge"])
    assert r["ratio_all"] <= A.gate(U.RATIO_MEASURED["ratio_all"])
    assert r["edge_resolved"] < r["edge_b"]
