"""Adaptive sampling without a GPU: the C-ABI additions (symbols, the struct's
layout by the gcc offset harness, the defaults, the rejections that need no context), the numpy
restatement of the plan step (tests/adaptive_ref.py) and the invariants it must keep on random and
adversarial inputs, the scene-specialised module's source tag, key and compilation with the map,
and the premise of the GPU parity tests on the oracle's side: a pixel of the oracle's frame at
spp = s is that pixel rendered alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import denoise_ref as R
import oracle as O
import rvcp_amd
from conftest import ROOT
from rvcp_amd import abi

HEADER = os.path.join(ROOT, "include", "rvcp.h")
NEW_SYMBOLS = ("rvcp_render_spp_map_async", "rvcp_adaptive_params_default", "rvcp_spp_plan_async",
               "rvcp_spp_plan_wait", "rvcp_set_adaptive", "rvcp_get_adaptive",
               "rvcp_adaptive_last_map")
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("pad", "<f4", 3)])
f32 = np.float32


# ------------------------------------------------------------------------------ the interface
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
    assert isinstance(rvcp_amd.RayTracer.adaptive, property)
    for m in ("render_spp_map_async", "spp_plan_async", "spp_plan_wait", "adaptive_last_map"):
        assert callable(getattr(rvcp_amd.RayTracer, m)), m
    assert "#define RVCP_SPP_MAP_MAX 256u" in open(HEADER).read()
    assert abi.SPP_MAP_MAX == A.SPP_MAP_MAX == 256
    assert L.rvcp_abi_version() == abi.ABI_VERSION == 2                 # the ABI did not move


LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
  printf("rvcp_adaptive_params_t %zu\n", sizeof(rvcp_adaptive_params_t));
  F(rvcp_adaptive_params_t, spp_min); F(rvcp_adaptive_params_t, spp_max);
  F(rvcp_adaptive_params_t, mean_spp); F(rvcp_adaptive_params_t, weight_cap);
  F(rvcp_adaptive_params_t, epsilon); F(rvcp_adaptive_params_t, _pad);
  return 0;
}
"""


def test_params_layout_matches_the_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    dt = abi.ADAPTIVE_PARAMS_DTYPE
    assert c["rvcp_adaptive_params_t"] == dt.itemsize == 24
    assert [c[f"rvcp_adaptive_params_t.{n}"] for n in dt.names] == [dt.fields[n][1] for n in dt.names]
    assert dt.names == ("spp_min", "spp_max", "mean_spp", "weight_cap", "epsilon", "_pad")


def test_defaults():
    p = abi.make_adaptive_params()
    assert abi.load().rvcp_adaptive_params_default(None) == abi.RVCP_E_INVALID
    for k, v in A.DEFAULTS.items():
        assert f32(p[k]) == f32(v), k
    assert 1 <= p["spp_min"] <= p["mean_spp"] <= p["spp_max"] <= abi.SPP_MAP_MAX
    assert p["weight_cap"] > 0 and p["epsilon"] > 0 and p["_pad"] == 0
    assert abi.make_adaptive_params(spp_max=32)["spp_max"] == 32


def test_null_context_is_rejected_without_a_device():
    L = abi.load()
    p = ctypes.c_void_p(1)
    prm = abi.make_adaptive_params()
    assert L.rvcp_render_spp_map_async(None, p, 64, 64, p, 4, p, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_spp_plan_async(None, p, p, p, p, 8, 8, abi.ptr(prm), p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_spp_plan_wait(None, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_set_adaptive(None, abi.ptr(prm)) == abi.RVCP_E_INVALID
    assert L.rvcp_get_adaptive(None, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_adaptive_last_map(None, None, None, None) == abi.RVCP_E_INVALID


# --------------------------------------------------------------------------- the restatement
def _case(W, H, seed, misses=True):
    """Random variance / colour / length planes under denoise_ref's synthetic guides."""
    rng = np.random.default_rng(seed)
    _, g = R.synthetic_case(W, H, seed)
    if not misses:
        g["face"] = 7
        g["material"] = 1
    lin = rng.uniform(0, 2, (H, W, 3)).astype(f32) * (rng.random((H, W, 1)) < 0.8)
    var = (rng.uniform(0, 1, (H, W)) ** 4).astype(f32) * f32(0.5)
    n = rng.integers(0, 34, (H, W)).astype(np.uint32)
    return var, lin, n, g


def _check_invariants(m, total, prm, npx):
    B, _ = A.budget(prm["mean_spp"], prm["spp_min"], npx)
    assert m.dtype == np.uint32 and total == int(m.astype(np.uint64).sum())
    assert total <= B, (total, B)
    assert m.min() >= prm["spp_min"] and m.max() <= prm["spp_max"]


@pytest.mark.parametrize("prm", [dict(), dict(spp_min=2, spp_max=5, mean_spp=3.5),
                                 dict(spp_min=1, spp_max=256, mean_spp=31.25, weight_cap=0.01),
                                 dict(spp_min=4, spp_max=4, mean_spp=4.0),
                                 dict(weight_cap=1e-6, epsilon=1e-9),
                                 dict(spp_min=256, spp_max=256, mean_spp=256.0)])
@pytest.mark.parametrize("W,H", [(67, 45), (130, 3), (8, 8), (1, 1), (64, 8), (65, 9)])
def test_budget_and_bounds_hold_on_random_frames(W, H, prm):
    prm = dict(A.DEFAULTS, **prm)
    for seed in range(3):
        var, lin, n, g = _case(W, H, 100 * seed + W)
        for length in (n, None):
            m, total = A.plan(var, lin, length, g, prm)
            assert m.shape == (H, W)
            _check_invariants(m, total, prm, W * H)


def test_a_pixel_that_asks_for_nothing_gets_the_minimum():
    """q = 0: a miss, an emissive texel, NaN / inf / negative / zero variance, a non-finite colour,
    a history of length 0; where anything else asks, such a pixel gets exactly spp_min."""
    W, H = 16, 4
    var, lin, n, g = _case(W, H, 5, misses=False)
    var[:], n[:] = f32(0.01), 3
    lin[:] = f32(0.5)
    bad = {}
    g["face"][0, 0] = R.MISS; bad["miss"] = (0, 0)
    g["material"][0, 1] |= np.uint32(R.EMISSIVE); bad["emissive"] = (0, 1)
    var[0, 2] = np.nan; bad["nan v"] = (0, 2)
    var[0, 3] = np.inf; bad["inf v"] = (0, 3)
    var[0, 4] = -1.0; bad["negative v"] = (0, 4)
    var[0, 5] = 0.0; bad["zero v"] = (0, 5)
    var[0, 6] = -0.0; bad["minus zero v"] = (0, 6)
    lin[0, 7, 1] = np.nan; bad["nan colour"] = (0, 7)
    lin[0, 8, 2] = -np.inf; bad["inf colour"] = (0, 8)
    n[0, 9] = 0; bad["n = 0"] = (0, 9)
    q = A.priorities(var, lin, n, g, 1.0, 1e-4)
    for what, at in bad.items():
        assert q[at] == 0, what
    ok = np.ones((H, W), bool)
    for at in bad.values():
        ok[at] = False
    assert (q[ok] > 0).all() and len(set(q[ok].tolist())) == 1
    m, total = A.plan(var, lin, n, g, A.DEFAULTS)
    assert (m[~ok] == 1).all() and (m[ok] > 1).all()
    _check_invariants(m, total, A.DEFAULTS, W * H)
    # a position or a normal that is not finite is not read: the pixel still asks
    g["position"][1, 1] = np.nan
    g["normal"][1, 2] = np.inf
    assert np.array_equal(A.priorities(var, lin, n, g, 1.0, 1e-4), q)


def test_no_priority_anywhere_spreads_the_budget_evenly():
    """S == 0 (an all-miss frame, or nothing left to ask for): min(spp_min + E // npx, spp_max)."""
    W, H = 9, 7
    var, lin, n, g = _case(W, H, 9)
    g["face"] = R.MISS
    for prm, want in ((dict(), 4), (dict(mean_spp=4.99), 4), (dict(mean_spp=1.0), 1),
                      (dict(spp_min=2, spp_max=3, mean_spp=3.0), 3),
                      (dict(spp_min=3, spp_max=40, mean_spp=17.5), 17)):
        prm = dict(A.DEFAULTS, **prm)
        m, total = A.plan(var, lin, n, g, prm)
        assert (m == want).all(), prm
        _check_invariants(m, total, prm, W * H)
    g2 = _case(W, H, 9, misses=False)[3]
    m, _ = A.plan(np.zeros_like(var), lin, n, g2, A.DEFAULTS)
    assert (m == 4).all()


def test_priorities_saturate_at_the_cap():
    W, H = 8, 2
    var, lin, n, g = _case(W, H, 3, misses=False)
    n[:] = 1
    lin[:] = 0
    eps, cap = f32(1e-4), f32(0.5)
    var[:] = cap * eps * f32(0.25)                   # w = cap / 4
    var[0, 0] = cap * eps                            # w = cap exactly: t = 1
    var[0, 1] = cap * eps * f32(1000.0)              # far above: cut off
    var[0, 2] = f32(3e38)                            # r overflows to inf: cut off
    lin[0, 3] = f32(3e38)                            # l * l overflows: r = 0
    q = A.priorities(var, lin, n, g, cap, eps)
    assert q[0, 0] == q[0, 1] == q[0, 2] == 1 << 20
    assert q[0, 3] == 0
    assert q[1, 0] == 1 << 18
    assert q.max() == 1 << 20
    # the same relative variance over a longer history asks for less
    n[1, 1] = 4
    assert A.priorities(var, lin, n, g, cap, eps)[1, 1] == 1 << 16


def test_one_pixel_and_the_uniform_map():
    g = np.zeros((1, 1), R.GBUFFER_DTYPE)
    one = lambda v: (np.full((1, 1), v, f32), np.full((1, 1, 3), 0.5, f32), None, g)   # noqa: E731
    m, total = A.plan(*one(0.3), A.DEFAULTS)
    assert m.tolist() == [[4]] and total == 4        # the whole surplus: 1 + min(3 * q // q, 31)
    m, total = A.plan(*one(0.0), A.DEFAULTS)
    assert m.tolist() == [[4]] and total == 4        # S == 0
    m, _ = A.plan(*one(0.3), dict(A.DEFAULTS, spp_max=3, mean_spp=3.0))
    assert m.tolist() == [[3]]
    # mean_spp == spp_min: E = 0 and every pixel gets spp_min, whatever it asks for
    var, lin, n, gg = _case(33, 5, 1)
    for smin in (1, 3):
        prm = dict(A.DEFAULTS, spp_min=smin, mean_spp=float(smin))
        m, total = A.plan(var, lin, n, gg, prm)
        assert (m == smin).all() and total == smin * m.size
    assert A.uniform_count(A.DEFAULTS) == 4
    assert A.uniform_count(dict(A.DEFAULTS, mean_spp=2.75)) == 2
    assert A.uniform_count(dict(spp_min=3, spp_max=9, mean_spp=3.0)) == 3


def test_the_surplus_of_clamped_pixels_is_not_redistributed():
    """One pixel holds all the priority: it is clamped to spp_max and the rest stay at spp_min, so
    the frame spends less than its budget."""
    W, H = 8, 8
    var, lin, n, g = _case(W, H, 2, misses=False)
    var[:] = 0
    var[3, 3] = 1.0
    lin[:] = 0.5
    n[:] = 1
    m, total = A.plan(var, lin, n, g, A.DEFAULTS)
    assert m[3, 3] == 32 and (np.delete(m.ravel(), 3 * W + 3) == 1).all()
    assert total == 63 + 32 < A.budget(4.0, 1, 64)[0] == 256


def test_clamp_map():
    m = np.array([0, 1, 256, 300, 0xFFFFFFFF, 17], np.uint32)
    assert A.clamp_map(m).tolist() == [1, 1, 256, 256, 256, 17]


# ------------------------------------------------------------------ the specialised modules
def _cornell_records(cornell):
    v = cornell.mesh.aligned_vertices()["position"][:, :3]
    p = v[cornell.mesh.aligned_faces()["vertices"]].astype(np.float32)
    rec = np.zeros(len(p), dtype=TRI_DTYPE)
    rec["v0"] = p[:, 0]
    rec["e1"] = (p[:, 1] - p[:, 0]).astype(np.float32)
    rec["e2"] = (p[:, 2] - p[:, 0]).astype(np.float32)
    return rec


def _source(fn, rec, *mode):
    n = fn(rec.ctypes.data, len(rec), *mode, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    fn(rec.ctypes.data, len(rec), *mode, buf, n + 1)
    return buf.value.decode()


def test_map_module_source_and_key_are_its_own(cornell):
    """The map module's source tag and compile key differ from the default's and the cosine's; the
    default's and the cosine's are what the hooks of §4.17 report (no map: nothing added)."""
    L = abi.load()
    rec = _cornell_records(cornell)
    vp, u32, ci, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    src, src_map = L.rvcp_internal_jit_module_source, L.rvcp_internal_jit_module_source_map
    src.restype = src_map.restype = sz
    src.argtypes = [vp, u32, ci, ctypes.c_char_p, sz]
    src_map.argtypes = [vp, u32, ci, ci, ctypes.c_char_p, sz]
    key, key_map = L.rvcp_internal_jit_module_key_for, L.rvcp_internal_jit_module_key_for_map
    key.restype = key_map.restype = ctypes.c_uint64
    key.argtypes = [vp, u32, ci]
    key_map.argtypes = [vp, u32, ci, ci]
    sources, keys = {}, {}
    for mode in (abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE):
        plain = _source(src, rec, mode)
        assert _source(src_map, rec, mode, 0) == plain
        assert key_map(rec.ctypes.data, len(rec), mode, 0) == key(rec.ctypes.data, len(rec), mode)
        sources[mode, 0], keys[mode, 0] = plain, key(rec.ctypes.data, len(rec), mode)
        sources[mode, 1] = _source(src_map, rec, mode, 1)
        keys[mode, 1] = key_map(rec.ctypes.data, len(rec), mode, 1)
        assert sources[mode, 1].startswith(plain) and "spp_map" in sources[mode, 1][len(plain):]
        assert "spp_map" not in plain
    assert len(set(sources.values())) == 4 and len(set(keys.values())) == 4 and all(keys.values())


def test_map_module_compiles_for_gfx950(cornell):
    """hipRTC builds the Cornell box's module with -DRVCP_SPP_MAP=1 here, without a GPU, for both
    bounce samplings and with the BVH hybrid's kernels; the code object is not the default's."""
    rec = _cornell_records(cornell)
    fn = abi.load().rvcp_internal_jit_compile_check_map
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p, ctypes.c_size_t]
    sizes = {}
    for mode, spp_map, bvh in ((0, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1)):
        n = ctypes.c_size_t(0)
        err = ctypes.create_string_buffer(4096)
        rc = fn(rec.ctypes.data, len(rec), mode, spp_map, bvh, ctypes.byref(n), err, 4096)
        if rc != 0 and b"libhiprtc not found" in err.value:
            pytest.skip("hipRTC not installed")
        assert rc == 0, err.value.decode()
        sizes[mode, spp_map, bvh] = n.value
    assert min(sizes.values()) > 10000 and len(set(sizes.values())) == 4, sizes


# ------------------------------------------------------------------- the oracle-side premise
@pytest.mark.parametrize("spp", [1, 3, 8])
def test_a_pixel_of_the_oracle_is_the_pixel_rendered_alone(cornell, cornell_arrays, spp):
    """Nothing couples the oracle's pixels: pixel (x, y) of the full frame at spp = s equals the
    same pixel rendered alone (rect = (x, y, 1, 1)), so a frame traced with a per-pixel count can
    be checked pixel by pixel against the oracle's frames of each count."""
    W, H, t = 24, 18, 123.0
    cfg = abi.make_config(spp=spp)
    push = cornell.push_constant(t)
    lin, rgba, trav = O.render(cornell_arrays, push, cfg, W, H)
    rng = np.random.default_rng(spp)
    total = 0
    for x, y in [(0, 0), (W - 1, H - 1), (11, 2)] + [(int(rng.integers(W)), int(rng.integers(H)))
                                                     for _ in range(9)]:
        l1, r1, t1 = O.render(cornell_arrays, push, cfg, W, H, rect=(x, y, 1, 1))
        assert np.array_equal(l1[0, 0].view(np.uint32), lin[y, x].view(np.uint32)), (x, y)
        assert np.array_equal(r1[0, 0], rgba[y, x]), (x, y)
        total += t1
    assert 0 < total < trav
