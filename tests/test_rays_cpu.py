"""Ray queries without a GPU: the two records' layout, the exported symbols,
the unchanged ABI revision, and the reference of tests/rays_ref.py against two independent
restatements of the scan -- tests/pyref.py and the brute column of tools/bvh4_check.cpp."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bvh_adversarial as A
import oracle
import pyref
import rays_ref
from conftest import ROOT
from rvcp_amd import abi

HEADER = os.path.join(ROOT, "include", "rvcp.h")
CSRC = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc")
SYMBOLS = ("rvcp_trace_rays_async", "rvcp_rays_wait", "rvcp_trace_rays", "rvcp_primary_rays_async",
           "rvcp_pick")

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "rvcp.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
#define S(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  S(rvcp_ray_t); F(rvcp_ray_t, origin); F(rvcp_ray_t, direction); F(rvcp_ray_t, t_min); F(rvcp_ray_t, t_max);
  S(rvcp_ray_hit_t); F(rvcp_ray_hit_t, face); F(rvcp_ray_hit_t, t); F(rvcp_ray_hit_t, b1); F(rvcp_ray_hit_t, b2);
  printf("RVCP_RAYS_NEAREST %d\nRVCP_RAYS_ANY %d\n", RVCP_RAYS_NEAREST, RVCP_RAYS_ANY);
  return 0;
}
"""


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("rays_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


def test_record_layouts(c_layout):
    assert c_layout["rvcp_ray_t"] == 32 and c_layout["rvcp_ray_hit_t"] == 16
    want = {"rvcp_ray_t.origin": 0, "rvcp_ray_t.direction": 12, "rvcp_ray_t.t_min": 24,
            "rvcp_ray_t.t_max": 28, "rvcp_ray_hit_t.face": 0, "rvcp_ray_hit_t.t": 4,
            "rvcp_ray_hit_t.b1": 8, "rvcp_ray_hit_t.b2": 12}
    for k, off in want.items():
        assert c_layout[k] == off, k
    # the numpy records: the binding's, the reference's and the adversarial generator's
    for dt in (abi.RAY_DTYPE, rays_ref.RAY_DTYPE, A.RAY_DTYPE):
        assert dt.itemsize == 32 and dt.names == ("o", "d", "t_min", "t_max")
        assert [dt.fields[n][1] for n in dt.names] == [0, 12, 24, 28]
        assert all(dt.fields[n][0].base == np.dtype("<f4") for n in dt.names)
    for dt in (abi.RAY_HIT_DTYPE, rays_ref.RAY_HIT_DTYPE):
        assert dt.itemsize == 16 and dt.names == ("face", "t", "b1", "b2")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
        assert dt.fields["face"][0] == np.dtype("<i4")
    assert (abi.RAYS_NEAREST, abi.RAYS_ANY) == (c_layout["RVCP_RAYS_NEAREST"], c_layout["RVCP_RAYS_ANY"]) == (0, 1)


def test_library_exports_the_five_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported
    assert set(SYMBOLS) <= set(abi.EXPORTED)
    L = abi.load()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None


def test_abi_revision_and_version_string_unchanged():
    m = re.search(r"#define RVCP_ABI_VERSION (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == abi.ABI_VERSION == 2
    L = abi.load()
    assert L.rvcp_abi_version() == 2
    assert L.rvcp_version() == b"rvcp-mi355x 0.3.0 (gfx950, ABI 2)"


def test_null_context_is_invalid():
    L = abi.load()
    p = abi.ptr(np.zeros(64, np.uint8))
    assert L.rvcp_trace_rays_async(None, p, 1, 0, p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_rays_wait(None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_trace_rays(None, p, 1, 0, p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_primary_rays_async(None, p, 4, 4, p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_pick(None, p, 4, 4, 0, 0, p) == abi.RVCP_E_INVALID


def cornell_rays(cornell, n_primary=30, n_inside=20):
    """Some 50 rays of the Cornell box: primary rays of a 37 x 23 frame, and seeded rays from
    inside the room in every direction."""
    rng = np.random.default_rng(0x5AE)
    push = cornell.push_constant(0.0)
    rows = [oracle.sample_ray(push, 37, 23, int(x), int(y))
            for x, y in zip(rng.integers(0, 37, n_primary), rng.integers(0, 23, n_primary))]
    for _ in range(n_inside):
        o = rng.uniform([-250.0, 20.0, -250.0], [250.0, 520.0, 250.0])
        d = rng.normal(size=3)
        rows.append(np.concatenate([o, d / np.linalg.norm(d), [0.01, 10000.0]]))
    return np.array(rows, np.float32).view(rays_ref.RAY_DTYPE).reshape(-1)


def test_reference_agrees_with_pyref(cornell, cornell_arrays):
    rays = cornell_rays(cornell)
    got = rays_ref.nearest(cornell_arrays, rays)
    sc = pyref.Scene(cornell_arrays["materials"], cornell_arrays["vertices"], cornell_arrays["faces"],
                     cornell_arrays["lum_face_ids"])
    F = np.float32
    hits = 0
    for r, g in zip(rays, got):
        o, d = pyref.v(*r["o"]), pyref.v(*r["d"])
        # scene_hit's loop, keeping the index it does not return
        face, bt = -1, F(r["t_max"])
        for i, f in enumerate(sc.faces):
            h = pyref.intersect(sc, o, d, F(r["t_min"]), bt, f)
            if h is not None and h[0] <= bt:
                bt, face = h[0], i
        best = pyref.scene_hit(sc, o, d, F(r["t_min"]), F(r["t_max"]), [0])
        assert int(g["face"]) == face
        if face >= 0:
            hits += 1
            assert F(g["t"]).view(np.uint32) == F(best[0]).view(np.uint32) == F(bt).view(np.uint32)
        else:
            assert g["t"] == 0 and g["b1"] == 0 and g["b2"] == 0
    assert hits >= len(rays) // 2       # (the room is open in front and the frame is wider: some miss)


def test_reference_agrees_with_the_checkers_brute_column(tmp_path):
    """The checker is built as tests/test_bvh_adversarial_cpu.py builds it, with
    -DBVH_CHECK_FUSED=1: its triangle test then forms dot and cross as the device and the oracle
    do (fused chains).  The default build multiplies and adds unfused -- a model
    consistent in itself, which is all the BVH-against-scan comparison needs -- and its brute
    column differs from the oracle's scan on 156 of these 588 rays (a few ulp of t on most,
    another face on the vertex- and edge-aimed ones)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    obj, exe = str(tmp_path / "rvcp_bvh.o"), str(tmp_path / "bvh4_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-c",
                    os.path.join(CSRC, "rvcp_bvh.cpp"), "-o", obj], check=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-DBVH_CHECK_FUSED=1",
                    os.path.join(ROOT, "tools", "bvh4_check.cpp"), obj, "-o", exe], check=True)
    mesh = A.ties_mesh()
    rays, _, _ = A.make_rays(mesh)
    res, _, p = A.run_checker(exe, mesh, rays, str(tmp_path))
    assert res is not None, p.stdout[-300:] + p.stderr[-300:]
    got = rays_ref.nearest(mesh.pos, rays)
    brute = res["brute"]
    assert np.array_equal(got["face"], brute["face"])
    hit = got["face"] >= 0
    assert hit.sum() >= 400
    assert np.array_equal(got["t"][hit].view(np.uint32), brute["t"][hit].view(np.uint32))


def test_non_finite_rays_miss_in_the_reference(cornell, cornell_arrays):
    rays = cornell_rays(cornell, 8, 0)
    ref = rays_ref.nearest(cornell_arrays, rays)
    for word in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = rays.copy()
            r.view(np.float32).reshape(-1, 8)[3, word] = bad
            got = rays_ref.nearest(cornell_arrays, r)
            assert got[3]["face"] == -1
            assert np.array_equal(np.delete(got, 3), np.delete(ref, 3))
