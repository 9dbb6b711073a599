"""G-buffer + a-trous denoiser, the part that needs no GPU: struct layouts, the binding, and the
numpy restatement of the filter (tests/denoise_ref.py) held to the filter's exact invariants and
to the quality gate of DESIGN.md §4.9."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import oracle as O
import rvcp_amd
from rvcp_amd import abi
from conftest import ROOT, scene_arrays

HEADER = os.path.join(ROOT, "include", "rvcp.h")

# the gcc offsetof harness of test_layout_abi.py, for the two new structs
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
#define S(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  S(rvcp_gbuffer_texel_t); F(rvcp_gbuffer_texel_t, position); F(rvcp_gbuffer_texel_t, face);
  F(rvcp_gbuffer_texel_t, normal); F(rvcp_gbuffer_texel_t, material);
  S(rvcp_denoise_params_t); F(rvcp_denoise_params_t, iterations);
  F(rvcp_denoise_params_t, normal_power_log2); F(rvcp_denoise_params_t, sigma_color);
  F(rvcp_denoise_params_t, sigma_plane);
  printf("MISS %u\nEMISSIVE %u\nMAX_ITERATIONS %d\n", RVCP_GBUFFER_MISS, RVCP_GBUFFER_EMISSIVE,
         RVCP_DENOISE_MAX_ITERATIONS);
  return 0;
}
"""

NEW_SYMBOLS = ("rvcp_render_gbuffer_async", "rvcp_denoise_params_default", "rvcp_denoise_async",
               "rvcp_denoise_wait", "rvcp_render_denoised")


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


# ---------------------------------------------------------------------------- layout
def test_gbuffer_texel_layout(c_layout):
    assert c_layout["rvcp_gbuffer_texel_t"] == 32
    assert c_layout["rvcp_gbuffer_texel_t.position"] == 0
    assert c_layout["rvcp_gbuffer_texel_t.face"] == 12
    assert c_layout["rvcp_gbuffer_texel_t.normal"] == 16
    assert c_layout["rvcp_gbuffer_texel_t.material"] == 28
    assert c_layout["MISS"] == abi.GBUFFER_MISS == R.MISS
    assert c_layout["EMISSIVE"] == abi.GBUFFER_EMISSIVE == R.EMISSIVE
    assert c_layout["MAX_ITERATIONS"] == abi.DENOISE_MAX_ITERATIONS == 8


def test_numpy_dtypes_match_header(c_layout):
    for cname, dt in (("rvcp_gbuffer_texel_t", abi.GBUFFER_DTYPE),
                      ("rvcp_denoise_params_t", abi.DENOISE_PARAMS_DTYPE),
                      ("rvcp_gbuffer_texel_t", R.GBUFFER_DTYPE)):
        assert dt.itemsize == c_layout[cname], cname
        for field in dt.names:
            assert dt.fields[field][1] == c_layout[f"{cname}.{field}"], (cname, field)


# ---------------------------------------------------------------------------- binding
def test_library_exports_the_new_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW_SYMBOLS if f not in exported]
    L = abi.load()
    for f in NEW_SYMBOLS:
        assert f in abi.EXPORTED
        assert getattr(L, f).argtypes is not None, f       # declared by abi.load()


def test_denoise_params_default_needs_no_gpu():
    L = abi.load()
    p = np.zeros((), dtype=abi.DENOISE_PARAMS_DTYPE)
    assert L.rvcp_denoise_params_default(abi.ptr(p)) == abi.RVCP_OK
    assert 1 <= int(p["iterations"]) <= abi.DENOISE_MAX_ITERATIONS
    assert 0 <= int(p["normal_power_log2"]) <= 8
    assert float(p["sigma_color"]) > 0 and float(p["sigma_plane"]) > 0
    assert L.rvcp_denoise_params_default(None) == abi.RVCP_E_INVALID
    assert abi.make_denoise_params().tobytes() == p.tobytes()
    q = abi.make_denoise_params(iterations=2, sigma_color=float("inf"))
    assert int(q["iterations"]) == 2 and np.isinf(q["sigma_color"])
    assert q["sigma_plane"] == p["sigma_plane"]


def test_new_entry_points_reject_a_null_context():
    L = abi.load()
    import ctypes
    p = ctypes.c_void_p(1)
    assert L.rvcp_render_gbuffer_async(None, p, 8, 8, p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_denoise_async(None, p, p, 8, 8, None, p, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_denoise_wait(None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_render_denoised(None, p, 8, 8, None, p, None, None, None) == abi.RVCP_E_INVALID


def test_run_headless_denoise_argument():
    """interactive.run_headless: the default renders as before (tracer.render, three
    arguments); with params every frame goes through tracer.render_denoised."""
    from rvcp_amd import interactive

    class Stub:
        def __init__(self):
            self.calls = []

        def render(self, *a):
            self.calls.append(("render", a))
            return np.zeros((4, 4, 4), np.uint8)

        def render_denoised(self, *a):
            self.calls.append(("render_denoised", a))
            return np.zeros((4, 4, 4), np.uint8)

    sc = rvcp_amd.Scene.default()
    t = Stub()
    interactive.run_headless(t, sc, 2, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0 + i)
    assert t.calls == [("render", (4, 4, 3.0)), ("render", (4, 4, 4.0))]
    t, p = Stub(), abi.make_denoise_params(iterations=1)
    interactive.run_headless(t, sc, 1, 4, 4, fixed_dt=0.01, time_seed=lambda i: 3.0, denoise=p)
    assert [c[0] for c in t.calls] == ["render_denoised"] and t.calls[0][1][:3] == (4, 4, 3.0)
    assert t.calls[0][1][3] is p


# ---------------------------------------------------------------------------- exact invariants
PARAM_SETS = [dict(iterations=3, normal_power_log2=5, sigma_color=1.0, sigma_plane=1.0),
              dict(iterations=5, normal_power_log2=0, sigma_color=float("inf"), sigma_plane=0.25)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kw", PARAM_SETS)
def test_half_planes_do_not_mix(kw):
    """w_n is exactly 0 across perpendicular normals, and sum(w * 1) / sum(w) is exactly 1."""
    c, g, left = R.half_planes()
    out = R.denoise(c, g, **kw)
    assert np.all(bits(out[left]) == bits(np.float32(0.0)))
    assert np.all(bits(out[~left]) == bits(np.float32(1.0)))


@pytest.mark.parametrize("kw", PARAM_SETS)
def test_non_filterable_pixels_pass_through_and_feed_nothing(kw):
    c, g = R.synthetic_case(45, 31, seed=3)
    filt = R.filterable(g)
    assert filt.any() and (g["face"] == R.MISS).any() and \
        ((g["material"] & np.uint32(R.EMISSIVE)) != 0).any()
    out = R.denoise(c, g, **kw)
    assert np.array_equal(bits(out[~filt]), bits(c[~filt]))
    assert np.isfinite(out[filt]).all()
    hot = c.copy()
    hot[~filt] = 1.0e30
    out_hot = R.denoise(hot, g, **kw)
    assert np.array_equal(bits(out_hot[filt]), bits(out[filt]))


@pytest.mark.parametrize("kw", PARAM_SETS)
def test_partition_of_unity(kw):
    """A constant colour on a coplanar patch comes back within 1e-5 relative.  One pass is a
    quotient of two sums over the same weights: at most 25 rounded products, 48 rounded
    additions and one division, 2^-24 each, about 4.5e-6 in the worst case -- asserted for every
    step on its own.  The chain is held to the same 1e-5 (its worst case would add up pass by
    pass; rounding errors of a weighted mean do not)."""
    c, g = R.coplanar_patch()
    rel = lambda out: np.abs(out.astype(np.float64) / c.astype(np.float64) - 1.0)   # noqa: E731
    for i in range(kw["iterations"]):
        one = R.atrous_pass(c, g, i, kw["normal_power_log2"], kw["sigma_color"], kw["sigma_plane"])
        assert np.all(rel(one) <= 1e-5), i
    assert np.all(rel(R.denoise(c, g, **kw)) <= 1e-5)


# ---------------------------------------------------------------------------- quality
@pytest.mark.slow
def test_quality_gate_cornell_64_spp4():
    """Cornell box 64^2 SPP = 4 against the oracle at SPP = 2048 (filterable pixels, colour
    clamped to [0, 1]): the restatement at the library's defaults must reach the gate of
    DESIGN.md §4.9.  Measured: RMSE 0.1374 -> 0.0404, ratio 0.294 (RATIO_MEASURED); gate 0.4705."""
    W = H = 64
    sc = rvcp_amd.Scene.default()
    g = R.cornell_gbuffer(W, H)
    mask = R.filterable(g)
    assert 0.90 < mask.mean() < 0.97            # 6.6 % miss / light pixels at this camera
    noisy, _, _ = O.render(scene_arrays(sc), sc.push_constant(5.0), abi.make_config(spp=4), W, H)
    ref = R.cornell_reference(W, H)
    out = R.denoise_params(noisy, g, abi.make_denoise_params())
    before, after = R.rmse(noisy, ref, mask), R.rmse(out, ref, mask)
    print(f"rmse noisy {before:.4f} denoised {after:.4f} ratio {after / before:.4f} "
          f"gate {R.QUALITY_GATE:.4f}")
    assert 0.0 < R.QUALITY_GATE < 1.0
    assert after <= R.QUALITY_GATE * before
