"""SVGF, the part that needs no GPU: the struct layout, the defaults and the
exported symbols; the numpy restatement (tests/svgf_ref.py) held against the two restatements it
extends (temporal_ref for the accumulation's colour and length, denoise_ref for the tap loop), to
the statistics of its variance estimate, to the quality gate with its two yardsticks and to the
edge it must keep where the plain a-trous filter blurs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import svgf_ref as S
import temporal_ref as T
import oracle as O
import rvcp_amd
from rvcp_amd import abi
from conftest import ROOT, scene_arrays

HEADER = os.path.join(ROOT, "include", "rvcp.h")
f32 = np.float32

FIELDS = ("iterations", "normal_power_log2", "sigma_luminance", "sigma_plane", "epsilon",
          "alpha_moments_min", "spatial_below", "_pad")
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
  printf("rvcp_svgf_params_t %zu\n", sizeof(rvcp_svgf_params_t));
""" + "".join(f"  F(rvcp_svgf_params_t, {f});\n" for f in FIELDS) + r"""
  printf("FEEDBACK %u\nMAX_ITERATIONS %u\nMAX_SPATIAL_BELOW %u\nABI %u\n", RVCP_SVGF_FEEDBACK,
         (unsigned)RVCP_SVGF_MAX_ITERATIONS, RVCP_SVGF_MAX_SPATIAL_BELOW, RVCP_ABI_VERSION);
  return 0;
}
"""

NEW_SYMBOLS = ("rvcp_svgf_params_default", "rvcp_svgf_accumulate_async", "rvcp_svgf_filter_async",
               "rvcp_svgf_wait", "rvcp_render_svgf", "rvcp_svgf_reset")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- layout, binding
def test_struct_layout_matches_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["rvcp_svgf_params_t"] == 32
    for dt in (abi.SVGF_PARAMS_DTYPE, S.PARAMS_DTYPE):
        assert dt.itemsize == 32 and dt.names == FIELDS
        for field in FIELDS:
            assert dt.fields[field][1] == c[f"rvcp_svgf_params_t.{field}"], field
    assert c["FEEDBACK"] == abi.SVGF_FEEDBACK == S.FEEDBACK == 1
    assert c["MAX_ITERATIONS"] == abi.SVGF_MAX_ITERATIONS == 8
    assert c["MAX_SPATIAL_BELOW"] == abi.SVGF_MAX_SPATIAL_BELOW == 16
    # only functions and one struct were added: the ABI revision and the version string stay
    assert c["ABI"] == abi.ABI_VERSION == 2
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
    for name in ("render_svgf", "render_svgf_push", "svgf_accumulate_async", "svgf_filter_async",
                 "svgf_wait", "svgf_reset"):
        assert callable(getattr(rvcp_amd.RayTracer, name))


def test_defaults_need_no_gpu():
    L = abi.load()
    p = np.zeros((), dtype=abi.SVGF_PARAMS_DTYPE)
    p["_pad"] = 7
    assert L.rvcp_svgf_params_default(abi.ptr(p)) == abi.RVCP_OK
    assert L.rvcp_svgf_params_default(None) == abi.RVCP_E_INVALID
    assert p.tobytes() == abi.make_svgf_params().tobytes() == S.params().tobytes()
    assert {k: p[k].item() for k in FIELDS} == dict(
        iterations=3, normal_power_log2=7, sigma_luminance=1.0, sigma_plane=f32(0.1).item(),
        epsilon=f32(1.0e-4).item(), alpha_moments_min=f32(0.05).item(), spatial_below=4, _pad=0)
    d = abi.make_denoise_params()
    assert p["sigma_plane"] == d["sigma_plane"] and p["normal_power_log2"] == d["normal_power_log2"]
    q = abi.make_svgf_params(sigma_luminance=float("inf"), spatial_below=1)
    assert np.isinf(q["sigma_luminance"]) and int(q["spatial_below"]) == 1 and int(q["iterations"]) == 3


def test_new_entry_points_reject_a_null_context():
    L = abi.load()
    p = ctypes.c_void_p(1)
    E = abi.RVCP_E_INVALID
    assert L.rvcp_svgf_accumulate_async(None, None, p, p, None, None, None, None, 8, 8, None, None,
                                        p, p, p, None, None) == E
    assert L.rvcp_svgf_filter_async(None, p, p, p, p, 8, 8, None, p, None, None, None, None) == E
    assert L.rvcp_svgf_wait(None, None, None) == E
    assert L.rvcp_svgf_reset(None) == E
    assert L.rvcp_render_svgf(None, p, 8, 8, None, None, 0, p, None, None, None, None, None, None) == E


def test_run_headless_svgf_argument():
    """interactive.run_headless: `svgf` takes precedence over `temporal` and `denoise`; without it
    nothing changes."""
    from rvcp_amd import interactive

    class Stub:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("render", "render_denoised", "render_temporal", "render_svgf"):
                raise AttributeError(name)

            def f(*a):
                self.calls.append((name, a))
                return np.zeros((4, 4, 4), np.uint8)
            return f

    sc = rvcp_amd.Scene.default()
    s, p, d = abi.make_svgf_params(), abi.make_temporal_params(), abi.make_denoise_params()
    t = Stub()
    interactive.run_headless(t, sc, 2, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0 + i, svgf=s)
    assert [c[0] for c in t.calls] == ["render_svgf"] * 2
    assert t.calls[1][1][:3] == (4, 4, 4.0) and t.calls[1][1][3] is None and t.calls[1][1][4] is s
    t = Stub()
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0, svgf=s,
                             temporal=p, denoise=d)
    assert [c[0] for c in t.calls] == ["render_svgf"]
    assert t.calls[0][1][3] is p and t.calls[0][1][4] is s
    t = Stub()
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0, temporal=p,
                             svgf=None)
    assert [c[0] for c in t.calls] == ["render_temporal"]
    t = Stub()
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0)
    assert t.calls == [("render", (4, 4, 3.0))]


# ---------------------------------------------------------------------------- against §4.10, §4.9
@pytest.mark.parametrize("mode", ["identity", "reprojection", "no_history"])
def test_accumulation_colour_and_length_equal_temporal_ref(mode):
    W, H = 45, 31
    tp = T.params(alpha_min=0.0, max_history=40, normal_min=0.8, sigma_plane=0.25)
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed=3, identity=mode == "identity", p=tp)
    pm = S.synthetic_moments(pc, seed=4)
    v = None if mode == "identity" else view
    if mode == "no_history":
        pc = pg = pl = pm = None
    want, want_len = T.accumulate(c, g, pc, pg, pl, v, tp)
    sp = S.params(alpha_moments_min=0.2)
    got, got_len, mom = S.accumulate(c, g, pc, pg, pl, pm, v, tp, sp)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_len, want_len)
    # the moments: (0, 0) off the filterable pixels, (l, l^2) where a history starts, the
    # history's blended in elsewhere; rejected history texels feed nothing
    filt = R.filterable(g)
    l1 = S.lum(c)
    mu = np.stack([l1, l1 * l1], axis=-1)
    assert not mom[~filt].any()
    fresh = filt & (got_len == 1) if mode == "no_history" else filt & np.all(bits(got) == bits(c), -1) & (got_len == 1)
    assert fresh.any() and np.array_equal(bits(mom[fresh]), bits(mu[fresh]))
    if pm is not None:
        cont = filt & (got_len > 1)
        assert cont.any() and (bits(mom[cont]) != bits(mu[cont])).any()
        hot = pm.copy()
        hot[~R.filterable(pg) | (pl == 0)] = 1.0e30
        assert np.array_equal(bits(S.accumulate(c, g, pc, pg, pl, hot, v, tp, sp)[2]), bits(mom))


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_guided_passes_without_the_luminance_weight_equal_denoise_ref(iterations):
    W, H = 45, 31
    c, g = R.synthetic_case(W, H, seed=9)
    rng = np.random.default_rng(1)
    v = (rng.random((H, W)) ** 2 * 50.0).astype(f32)
    sp = S.params(iterations=iterations, sigma_luminance=float("inf"), normal_power_log2=3,
                  sigma_plane=20.0)
    want = R.denoise(c, g, iterations, 3, float("inf"), 20.0)
    got, gv = c, v
    for i in range(iterations):
        got, gv = S.guided_pass(got, gv, g, i, sp)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(gv).all() and (gv >= 0).all() and not gv[~R.filterable(g)].any()


def test_variance_sanity():
    """v of B and v' of every pass: finite, >= 0, 0 on non-filterable pixels; with and without
    the spatial branch, on colours up to 10^4."""
    W, H = 45, 31
    tp = T.params()
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed=6, p=tp)
    c = (c * f32(100.0)).astype(f32)
    pm = S.synthetic_moments(pc, seed=7)
    for below in (1, 4):
        sp = S.params(spatial_below=below, iterations=5, sigma_luminance=2.0)
        a, n, m = S.accumulate(c, g, pc, pg, pl, pm, view, tp, sp)
        v = S.variance(m, n, g, sp)
        filt = R.filterable(g)
        assert (filt & (n < below)).any() == (below > 1) and (filt & (n >= below)).any()
        planes = [v]
        col = a
        for i in range(5):
            col, v = S.guided_pass(col, v, g, i, sp)
            planes.append(v)
            assert np.isfinite(col).all()
            assert np.array_equal(bits(col[~filt]), bits(a[~filt]))
        for k, plane in enumerate(planes):
            assert plane.dtype == f32 and np.isfinite(plane).all() and (plane >= 0).all(), k
            assert not plane[~filt].any(), k
        assert planes[0][filt].max() > 0


# ---------------------------------------------------------------------------- the estimator
def noise_frames(n, seed=11):
    """n frames of i.i.d. uniform grey noise on denoise_ref.coplanar_patch (every pixel
    filterable, all geometric weights exactly 1): luminance variance 1/12 x (sum of the weights)^2."""
    _, g = R.coplanar_patch()
    rng = np.random.default_rng(seed)
    H, W = g.shape
    return [np.repeat(rng.random((H, W, 1)).astype(f32), 3, axis=-1) for _ in range(n)], g


def test_variance_estimator_is_the_biased_sample_variance():
    frames, g = noise_frames(16)
    tp = T.params(alpha_min=0.0, max_history=16)
    sp = S.params(alpha_moments_min=0.0, spatial_below=1)
    a = n = m = None
    for c in frames:
        a, n, m = S.accumulate(c, g, a, None if a is None else g, n, m, None, tp, sp)
    assert np.all(n == 16)
    v = S.variance(m, n, g, sp).astype(np.float64)
    ksum = float(S.LR) + float(S.LG) + float(S.LB)
    sigma2 = ksum * ksum / 12.0
    want = sigma2 * 15.0 / 16.0
    se = v.std(ddof=1) / np.sqrt(v.size)
    print(f"mean v {v.mean():.6f}, sigma^2 15/16 = {want:.6f}, standard error {se:.6f} "
          f"({abs(v.mean() - want) / se:.2f} se)")
    assert abs(v.mean() - want) <= 4.0 * se


def test_spatial_branch_on_the_first_frame():
    frames, g = noise_frames(1)
    tp = T.params()
    sp = S.params(spatial_below=4)
    a, n, m = S.accumulate(frames[0], g, None, None, None, None, None, tp, sp)
    assert np.all(n == 1)
    v = S.variance(m, n, g, sp)
    base = S.spatial_variance(m, g, sp)
    assert np.array_equal(bits(v), bits(base * f32(4.0)))
    inner = (slice(3, -3), slice(3, -3))
    assert (v[inner] > 0).all()
    # the unboosted estimate on the interior, where all 49 weights are exactly 1: the plain
    # float64 box statistic of the moments
    m64 = m.astype(np.float64)
    H, W = n.shape
    box = lambda x: sum(x[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx]                   # noqa: E731
                        for dy in range(-3, 4) for dx in range(-3, 4)) / 49.0
    want = box(m64[..., 1]) - box(m64[..., 0]) ** 2
    assert np.allclose(base[inner], want, rtol=1e-4, atol=1e-7)
    # with spatial_below = 1 the same frame has no variance at all (m2 = m1^2 up to rounding)
    assert S.variance(m, n, g, S.params(spatial_below=1)).max() < 1e-6


# ---------------------------------------------------------------------------- quality
@pytest.mark.slow
def test_quality_gate_and_yardsticks_cornell_64_spp4_8_frames():
    """The sweep's setup at the defaults: SVGF's 8th frame against the first raw frame (the gate)
    and against the two yardsticks computed here from the same frames."""
    W = H = 64
    sc = rvcp_amd.Scene.default()
    g = R.cornell_gbuffer(W, H)
    mask = R.filterable(g)
    ref = R.cornell_reference(W, H)
    tp, sp = abi.make_temporal_params(), abi.make_svgf_params()
    chain = S.Chain(tp, sp, feedback=False)
    acc = length = None
    first = None
    for t in S.QUALITY_SEEDS:
        noisy, _, _ = O.render(scene_arrays(sc), sc.push_constant(t), abi.make_config(spp=4), W, H)
        if first is None:
            first = R.rmse(noisy, ref, mask)
        out, var, n = chain.frame(noisy, g, None)
        acc, length = T.accumulate(noisy, g, acc, None if acc is None else g, length, None, tp)
    assert np.array_equal(n, length) and np.all(n[mask] == 8)
    after = R.rmse(out, ref, mask)
    y_temporal = R.rmse(acc, ref, mask)
    y_filtered = R.rmse(R.denoise_params(acc, g, abi.make_denoise_params()), ref, mask)
    print(f"rmse first raw {first:.4f} svgf {after:.4f} ratio {after / first:.4f} gate "
          f"{S.QUALITY_GATE:.4f}; temporal only {y_temporal:.4f}, temporal + a-trous defaults "
          f"{y_filtered:.4f}")
    assert 0.0 < S.QUALITY_GATE < 1.0
    assert after <= S.QUALITY_GATE * first
    assert after < y_temporal and after < y_filtered
    assert np.isfinite(var).all() and (var >= 0).all() and not var[~mask].any()


# ---------------------------------------------------------------------------- edge keeping
# Measured with this file: the fraction of a luminance step's contrast that is
# left after filtering 8 accumulated noisy frames.  Contrast: the difference of the means of the
# five columns next to the edge on either side, rows 5 .. H - 6.  The gate is the midpoint.
EDGE_KEPT_SVGF = 0.995
EDGE_KEPT_ATROUS = 0.651
EDGE_GATE = 0.5 * (EDGE_KEPT_SVGF + EDGE_KEPT_ATROUS)
EDGE_LOW, EDGE_HIGH, EDGE_NOISE = 0.2, 0.8, 0.2


def edge_case():
    _, g = R.coplanar_patch()
    H, W = g.shape
    rng = np.random.default_rng(21)
    base = np.where(np.arange(W) < W // 2, f32(EDGE_LOW), f32(EDGE_HIGH))[None, :, None]
    frames = [np.repeat((base + rng.uniform(-EDGE_NOISE, EDGE_NOISE, (H, W, 1))).astype(f32), 3, -1)
              for _ in range(8)]
    return frames, g


def edge_contrast(img):
    H, W = img.shape[:2]
    e = W // 2
    lum = S.lum(np.ascontiguousarray(img, dtype=f32)).astype(np.float64)[5:H - 5]
    return lum[:, e:e + 5].mean() - lum[:, e - 5:e].mean()


def test_a_luminance_step_on_one_plane_is_kept():
    frames, g = edge_case()
    tp, sp = T.params(), S.params()
    chain = S.Chain(tp, sp)
    acc = length = None
    for c in frames:
        out, _, _ = chain.frame(c, g, None)
        acc, length = T.accumulate(c, g, acc, None if acc is None else g, length, None, tp)
    plain = R.denoise_params(acc, g, abi.make_denoise_params())
    step = (EDGE_HIGH - EDGE_LOW) * (float(S.LR) + float(S.LG) + float(S.LB))
    kept, kept_plain = edge_contrast(out) / step, edge_contrast(plain) / step
    # both filters remove noise: the residual on the flat parts is below the accumulated frame's
    flat = (slice(5, -5), slice(3, 12))
    print(f"contrast kept: svgf {kept:.4f}, a-trous defaults {kept_plain:.4f}, gate {EDGE_GATE:.4f}; "
          f"flat-part std: accumulated {acc[flat].std():.4f} svgf {out[flat].std():.4f} "
          f"a-trous {plain[flat].std():.4f}")
    assert out[flat].std() < acc[flat].std()
    assert kept > kept_plain
    assert kept >= EDGE_GATE >= kept_plain
