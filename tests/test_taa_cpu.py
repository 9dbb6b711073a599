"""Temporal anti-aliasing without a GPU: the C-ABI additions (layout, symbols,
defaults, NULL rejection), the jitter against its float64 restatement, exact properties of the
float32 restatement of the resolve (tests/taa_ref.py), the ghosting check and the anti-aliasing
gate on CPU G-buffers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
import taa_ref as A
import rvcp_amd
from rvcp_amd import abi
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rvcp.h")
f32 = np.float32
SEED = 1

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
#define S(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  S(rvcp_taa_params_t); F(rvcp_taa_params_t, alpha_min); F(rvcp_taa_params_t, max_history);
  F(rvcp_taa_params_t, clamp); F(rvcp_taa_params_t, _pad);
  printf("PERIOD %u\nABI %u\n", RVCP_TAA_JITTER_PERIOD, RVCP_ABI_VERSION);
  return 0;
}
"""

NEW_SYMBOLS = ("rvcp_taa_jitter", "rvcp_taa_jitter_push", "rvcp_taa_params_default",
               "rvcp_taa_resolve_async", "rvcp_taa_wait", "rvcp_set_taa", "rvcp_get_taa",
               "rvcp_taa_reset")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("taa_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


# ---------------------------------------------------------------------------- layout, binding
def test_struct_layout_matches_header(c_layout):
    assert c_layout["rvcp_taa_params_t"] == 16
    for dt in (abi.TAA_PARAMS_DTYPE, A.PARAMS_DTYPE):
        assert dt.itemsize == 16
        for field in dt.names:
            assert dt.fields[field][1] == c_layout[f"rvcp_taa_params_t.{field}"], field
    assert c_layout["PERIOD"] == abi.TAA_JITTER_PERIOD == A.JITTER_PERIOD == 16
    # only functions, constants and one struct were added: the ABI revision stays
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
    for name in ("taa_resolve_async", "taa_wait", "taa_reset"):
        assert callable(getattr(rvcp_amd.RayTracer, name))
    assert isinstance(rvcp_amd.RayTracer.taa, property)
    assert callable(rvcp_amd.taa_jitter) and callable(rvcp_amd.taa_jitter_push)


def test_defaults_need_no_gpu():
    L = abi.load()
    p = np.zeros((), dtype=abi.TAA_PARAMS_DTYPE)
    p["_pad"] = 7
    assert L.rvcp_taa_params_default(abi.ptr(p)) == abi.RVCP_OK
    assert p["alpha_min"] == f32(0.1) and int(p["max_history"]) == 32
    assert int(p["clamp"]) == 1 and int(p["_pad"]) == 0
    assert L.rvcp_taa_params_default(None) == abi.RVCP_E_INVALID
    assert abi.make_taa_params().tobytes() == p.tobytes() == A.params().tobytes()
    q = abi.make_taa_params(alpha_min=0.0, clamp=0)
    assert q["alpha_min"] == 0 and int(q["clamp"]) == 0 and int(q["max_history"]) == 32


def test_new_entry_points_reject_null_arguments():
    L = abi.load()
    p = ctypes.c_void_p(1)
    E = abi.RVCP_E_INVALID
    assert L.rvcp_taa_resolve_async(None, None, None, p, p, None, None, 8, 8, None, p, p, None,
                                    None) == E
    assert L.rvcp_taa_wait(None, None) == E
    assert L.rvcp_taa_reset(None) == E
    assert L.rvcp_set_taa(None, 1) == E
    assert L.rvcp_get_taa(None, p) == E
    assert L.rvcp_taa_jitter(0, None) == E
    push = np.ascontiguousarray(rvcp_amd.Scene.default().push_constant(0.0)).reshape(())
    out = np.zeros_like(push)
    j = np.array([0.25, -0.25], dtype=f32)
    assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 8, abi.ptr(j), abi.ptr(out)) == abi.RVCP_OK
    assert L.rvcp_taa_jitter_push(None, 8, 8, abi.ptr(j), abi.ptr(out)) == E
    assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 8, None, abi.ptr(out)) == E
    assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 8, abi.ptr(j), None) == E
    assert L.rvcp_taa_jitter_push(abi.ptr(push), 0, 8, abi.ptr(j), abi.ptr(out)) == E
    assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 0, abi.ptr(j), abi.ptr(out)) == E
    for bad in ([np.nan, 0.0], [0.0, np.inf], [1.5, 0.0], [0.0, -1.0000001]):
        b = np.array(bad, dtype=f32)
        assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 8, abi.ptr(b), abi.ptr(out)) == E, bad
    for edge in ([1.0, -1.0], [-1.0, 1.0]):
        b = np.array(edge, dtype=f32)
        assert L.rvcp_taa_jitter_push(abi.ptr(push), 8, 8, abi.ptr(b), abi.ptr(out)) == abi.RVCP_OK
    bad_push = push.copy()
    bad_push["camera"]["up"][..., :3] = bad_push["camera"]["forward"]     # forward x up = 0
    assert L.rvcp_taa_jitter_push(abi.ptr(bad_push), 8, 8, abi.ptr(j), abi.ptr(out)) == E


def test_run_headless_has_the_taa_argument():
    import inspect
    from rvcp_amd import interactive as I
    assert inspect.signature(I.run_headless).parameters["taa"].default is None


# ---------------------------------------------------------------------------- the jitter
def test_jitter_table_is_halton_2_3_with_period_16():
    table = np.array([rvcp_amd.taa_jitter(i) for i in range(40)])
    assert table.dtype == f32 and table.shape == (40, 2)
    want = np.array([A.jitter(i) for i in range(40)]).astype(f32)       # rounded once
    assert np.array_equal(bits(table), bits(want))
    assert np.array_equal(table[:16], table[16:32]) and np.array_equal(table[:8], table[32:])
    assert len({tuple(r) for r in table[:16]}) == 16
    assert np.all(np.abs(table) < 0.5 + 1e-6)
    # Halton(2, 3), spelled out: i = 1, 2, 3
    assert np.allclose(table[:3], [[0.0, 1 / 3 - 0.5], [-0.25, 2 / 3 - 0.5], [0.25, 1 / 9 - 0.5]])
    assert np.array_equal(rvcp_amd.taa_jitter(2 ** 32 - 1), table[(2 ** 32 - 1) % 16])


def _ulps(a, b):
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("rotated", [False, True])
def test_jitter_push_within_one_ulp_of_float64(rotated):
    sc = rvcp_amd.Scene.default()
    if rotated:
        sc = rvcp_amd.scene.rotated_scene(sc)
    push = np.ascontiguousarray(sc.push_constant(3.0)).reshape(())
    for W, H in ((37, 23), (64, 64), (1024, 1024)):
        for j in [rvcp_amd.taa_jitter(i) for i in range(16)] + [np.array([1.0, -1.0], dtype=f32)]:
            out = np.asarray(rvcp_amd.taa_jitter_push(push, W, H, j)).reshape(())
            want = A.jitter_forward_f64(push, H, j)
            got = out["camera"]["forward"]
            # a component that is 0 in float64 up to rounding noise has no ulp to speak of
            big = np.abs(want) > 1e-6
            assert _ulps(got[big], want[big].astype(f32)) <= 1, (W, H, j)
            assert np.all(np.abs(got[~big].astype(np.float64) - want[~big]) < 1e-12)
            # everything else is untouched, and the length is kept
            rest = out.copy()
            rest["camera"]["forward"] = push["camera"]["forward"]
            assert rest.tobytes() == push.tobytes()
            assert abs(np.linalg.norm(got.astype(np.float64)) /
                       np.linalg.norm(push["camera"]["forward"].astype(np.float64)) - 1) < 1e-6
            if np.any(j != 0):
                assert got.tobytes() != push["camera"]["forward"].tobytes()
        zero = np.asarray(rvcp_amd.taa_jitter_push(push, W, H, [0.0, 0.0]))
        assert zero.tobytes() == push.tobytes()
        assert np.asarray(rvcp_amd.taa_jitter_push(push, W, H, [-0.0, 0.0])).tobytes() == push.tobytes()


def test_jitter_push_moves_the_centre_by_the_jitter():
    """The hit of the centre ray of the unjittered camera lands `jitter` pixels from the centre
    of the jittered one, with the opposite sign (the camera turns, the image shifts back)."""
    sc = rvcp_amd.Scene.default()
    push = np.ascontiguousarray(sc.push_constant(0.0)).reshape(())
    W, H = 37, 23
    cam = push["camera"]
    x = (cam["position"][:3].astype(np.float64) + 500.0 * cam["forward"].astype(np.float64))
    j = np.array([0.4, -0.3], dtype=f32)
    jp = np.asarray(rvcp_amd.taa_jitter_push(push, W, H, j)).reshape(())
    fx, fy, z, _ = T.project(T.view_of_push(jp, H), x.astype(f32), W, H)
    assert z > 0
    assert abs(fx - ((W - 1) / 2 - 0.4)) < 1e-3 and abs(fy - ((H - 1) / 2 + 0.3)) < 1e-3


# ---------------------------------------------------------------------------- the restatement
def test_generator_meets_its_mix():
    for W, H in ((67, 45), (130, 3), (70, 5), (8, 8), (64, 64)):
        A.synthetic_case(W, H, SEED)         # asserts inside


def test_identity_with_equal_history_and_frame_returns_it():
    rng = np.random.default_rng(5)
    W, H = 67, 45
    c, g, _, _, cv, pv = A.synthetic_case(W, H, SEED)
    frame = rng.random((H, W, 3)).astype(f32)
    ln = rng.integers(1, 70000, (H, W)).astype(np.uint32)
    for p in (A.params(), A.params(clamp=0), A.params(alpha_min=0.0)):
        for views in ((None, None), (cv, cv.copy())):       # byte-equal views are the identity
            out, n = A.resolve(frame, g, frame, ln, views[0], views[1], p)
            assert np.array_equal(bits(out), bits(frame))
            assert np.array_equal(n, np.minimum(ln.astype(np.int64) + 1, 32))


PARAM_SETS = [A.params(), A.params(clamp=0), A.params(max_history=1),
              A.params(alpha_min=0.0, max_history=40)]


@pytest.mark.parametrize("p", PARAM_SETS, ids=["defaults", "clamp_0", "max_history_1", "alpha_min_0"])
@pytest.mark.parametrize("mode", ["reprojection", "identity", "no_history"])
def test_exact_properties(p, mode):
    """With clamp on every clamped interior output lies within its 3 x 3 box, up to one ulp:
    out = h + alpha (cur - h) with h and cur inside [lo, hi] and 0 <= alpha <= 1.  d = fl(cur - h)
    is off by at most ulp(d) / 2 <= ulp(cur) / 2 (0 <= h, so |d| <= the larger of the two), alpha d
    rounds to at most |d|, so h + t lies within half an ulp of the interval between h and cur and
    its rounding within one ulp of it."""
    W, H = 67, 45
    c, g, pr, pl, cv, pv = A.synthetic_case(W, H, SEED, p)
    if mode == "identity":
        cv = pv = None
    if mode == "no_history":
        pr = pl = None
    out, n, info = A.resolve(c, g, pr, pl, cv, pv, p, True)
    cur, has = A.sat(c), info["has"]
    assert out.dtype == f32 and n.dtype == np.uint32 and not np.isnan(out).any()
    # no history: the displayed current colour, length 1
    assert np.array_equal(bits(out[~has]), bits(cur[~has])) and np.all(n[~has] == 1)
    if mode == "no_history":
        assert not has.any()
        return
    assert has.any() and (~has).any()
    assert np.all(n[has] >= 1) and np.all(n <= int(p["max_history"]))
    if int(p["max_history"]) == 1:
        # alpha = 1: h + (cur - h) is cur up to the two roundings (see the test below)
        assert np.all(n == 1)
        assert np.max(np.abs(out.astype(np.float64) - cur.astype(np.float64))) <= 2.0 ** -24
        assert np.mean(bits(out) == bits(cur)) > 0.9
        return
    lo, hi = info["lo"], info["hi"]
    inside = (out >= np.nextafter(lo, f32(-np.inf))) & (out <= np.nextafter(hi, f32(np.inf)))
    clamped = info["interior"] & has
    if int(p["clamp"]) == 1:
        assert np.all(inside[clamped])
        assert info["changed"].any() and not info["changed"][~info["interior"]].any()
        # border pixels are never clamped: some of them leave what their box would be
        border = has & ~info["interior"]
        blo, bhi = _replicated_box(cur)
        outside = np.any((out < blo - 1e-3) | (out > bhi + 1e-3), axis=-1)
        assert outside[border].any()
    else:
        assert not info["changed"].any()
        assert not np.all(inside[clamped])


def _replicated_box(s):
    """The 3 x 3 box with replicated border pixels (what the resolve does NOT use)."""
    H, W = s.shape[:2]
    pad = np.pad(s, ((1, 1), (1, 1), (0, 0)), mode="edge")
    stack = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return stack.min(axis=0), stack.max(axis=0)


def test_max_history_1_returns_cur_up_to_rounding():
    """max_history = 1 makes alpha 1 and out = h + (cur - h).  That is cur in exact arithmetic; in
    float32 both operations round: d = fl(cur - h) is off by at most ulp(d) / 2 <= 2^-25 (|d| <= 1)
    and the sum, which lies within that of cur <= 1, by at most another 2^-25.  So the output is
    cur within 2^-24 absolute, and bit for bit wherever cur / 2 <= h <= 2 cur (the difference is
    exact there, Sterbenz)."""
    rng = np.random.default_rng(11)
    h = np.concatenate([rng.random(20000), [0.0, 1.0, 1e-30, 2.0 ** -24]]).astype(f32)
    cur = np.concatenate([rng.random(20000) ** 8, [1.0, 0.0, 1.0, 1.0]]).astype(f32)
    frame = np.stack([cur, cur, cur], axis=-1).reshape(1, -1, 3)
    hist = np.stack([h, h, h], axis=-1).reshape(1, -1, 3)
    g = np.zeros((1, frame.shape[1]), dtype=R.GBUFFER_DTYPE)
    out, n = A.resolve(frame, g, hist, np.full((1, frame.shape[1]), 9, dtype=np.uint32), None, None,
                       A.params(max_history=1))
    assert np.all(n == 1)
    assert np.array_equal(bits(out[0, :, 0]), bits(h + (cur - h)))
    err = np.abs(out[0, :, 0].astype(np.float64) - cur.astype(np.float64))
    assert err.max() <= 2.0 ** -24
    near = (h <= 2 * cur) & (2 * h >= cur)
    assert near.sum() > 1000 and np.array_equal(bits(out[0, near, 0]), bits(cur[near]))


# ---------------------------------------------------------------------------- ghosting
def test_ghosting_check():
    """The history is one constant colour absent from the frame, the camera moves by
    (60, 20, 0): one resolve with the clamp leaves every interior pixel inside its 3 x 3 box,
    without it the ghost stays."""
    W, H = 37, 23
    sc = rvcp_amd.Scene.default()
    g = R.cornell_gbuffer(W, H)
    c = A.flat_shade(g, sc.aligned_materials())
    ghost = np.empty((H, W, 3), dtype=f32)
    ghost[...] = (0.05, 0.9, 0.45)
    assert not np.any(np.all(np.isclose(A.sat(c), ghost[0, 0], atol=0.02), axis=-1))
    ln = np.full((H, W), 8, dtype=np.uint32)
    prev_push = np.ascontiguousarray(sc.push_constant(0.0)).reshape(())
    cur_push = prev_push.copy()
    cur_push["camera"]["position"][:3] += np.array([60.0, 20.0, 0.0], dtype=f32)
    cv, pv = T.view_of_push(cur_push, H), T.view_of_push(prev_push, H)
    on, _, info = A.resolve(c, g, ghost, ln, cv, pv, A.params(clamp=1), True)
    off, _ = A.resolve(c, g, ghost, ln, cv, pv, A.params(clamp=0))
    m = info["interior"] & info["has"]
    assert m.sum() > 0.5 * W * H
    lo, hi = info["lo"], info["hi"]
    inside = lambda o: np.all((o >= np.nextafter(lo, f32(-np.inf))) &      # noqa: E731
                              (o <= np.nextafter(hi, f32(np.inf))), axis=-1)
    assert np.all(inside(on)[m])
    assert not np.all(inside(off)[m])
    assert not np.array_equal(bits(on), bits(off))
    # the ghost's share of the unclamped frame is 1 - alpha = 8 / 9
    flat = m & np.all(hi - lo < 1e-6, axis=-1)
    assert flat.any()
    assert np.allclose(off[flat], ghost[flat] + (A.sat(c)[flat] - ghost[flat]) / 9, atol=1e-6)
    assert np.allclose(on[flat], A.sat(c)[flat], atol=1e-6)


# ---------------------------------------------------------------------------- the gate
@pytest.mark.slow
def test_anti_aliasing_gate_cornell_37x23():
    """16 jittered frames of the flat-shaded Cornell box resolved at the defaults, against the
    4 x 4 supersampled frame: the edge pixels' RMSE must fall to RATIO_MEASURED plus a quarter of
    the distance to 1 of a single centred frame's, and the other pixels must stay below the
    resolved edge RMSE."""
    sc = rvcp_amd.Scene.default()
    r = A.aa_gate(37, 23, np.ascontiguousarray(sc.push_constant(0.0)).reshape(()),
                  sc.aligned_materials(), A.cpu_gbuffer_of)
    print("\nTAA gate 37x23 (CPU G-buffers):", r)
    assert r["n_edge"] >= 100
    assert r["ratio"] <= A.gate(A.RATIO_MEASURED[(37, 23)])
    assert r["nonedge_resolved"] < r["edge_resolved"]
