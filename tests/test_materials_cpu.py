"""The material scattering mode's restatement (tests/materials_ref.py) on the
CPU: pinned to pyref.trace where nothing is specular, every kind of event met on the test frame,
the committed fixture equal to it, the bounded metal retry and the mirror's unbiasedness."""
import functools
import os

import numpy as np
import pytest

import materials_ref as M
import paths_ref
import pyref
import rvcp_amd
from rvcp_amd import abi

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "materials_frames.npz")


@functools.lru_cache(maxsize=None)
def frame(case):
    ev = M.new_events()
    lin, trav = M.case_frame(case, ev)
    lin.setflags(write=False)
    trav.setflags(write=False)
    return lin, trav, ev


@functools.lru_cache(maxsize=None)
def mirror():
    lin, trav = M.mirror_result()
    lin.setflags(write=False)
    return lin, trav


@pytest.mark.parametrize("which", ["cornell", "rotated"])
def test_equals_pyref_where_nothing_is_specular(which):
    sc = rvcp_amd.Scene.default()
    if which == "rotated":
        sc = rvcp_amd.scene.rotated_scene(sc)
    cfg = abi.make_config(spp=2)
    push = sc.push_constant(M.FIXTURE_TIME)
    ev = M.new_events()
    got, got_trav = M.render(sc, cfg, push, 24, 16, ev)
    want, want_trav = M.render(sc, cfg, push, 24, 16, trace_fn=pyref.trace)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_trav, want_trav)
    assert ev["lambertian_hits"] > 0
    assert all(ev[k] == 0 for k in M.EVENTS if k != "lambertian_hits")


def test_the_test_frame_meets_every_event():
    _, _, ev = frame("default")
    print(ev)
    for k in M.EVENTS:
        assert ev[k] >= 1, k


@pytest.mark.parametrize("case", list(M.CASES))
def test_fixture_equals_the_restatement(case):
    lin, trav, ev = frame(case)
    d = np.load(GOLDEN)
    assert np.array_equal(d[case + "/linear"].view(np.uint32), lin.view(np.uint32))
    assert np.array_equal(d[case + "/traversals_px"], trav)
    assert int(d[case + "/traversals"]) == int(trav.sum(dtype=np.uint64))
    assert [int(x) for x in d[case + "/events"]] == [ev[k] for k in M.EVENTS]


def test_the_metal_box_has_long_specular_chains():
    _, _, ev = frame("metal_box")
    assert ev["metal_redraws"] >= 16 and ev["metal_hits"] > 16 * 12


def test_mirror_fixture_equals_the_restatement():
    lin, trav = mirror()
    d = np.load(GOLDEN)
    assert np.array_equal(d["mirror/linear"].view(np.uint32), lin.view(np.uint32))
    assert np.array_equal(d["mirror/traversals"], trav)


def test_metal_retry_is_bounded():
    """A generator whose every draw fails: after METAL_RETRIES draws the direction is
    normalize(r), and exactly that many unit-ball samples were consumed."""
    n = pyref.v(0, 1, 0)
    r = pyref.reflect(pyref.v(0.6, -0.8, 0.0), n)
    assert pyref.dot(r, n) > 0
    draws = []

    def draw():
        draws.append(1)
        return pyref.v(0.0, -0.99, 0.0)       # r + 1 * (0, -1, 0) points below the surface

    ev = M.new_events()
    nd = M.metal_direction(r, n, F(1.0), draw, ev)
    assert len(draws) == M.METAL_RETRIES == 16
    assert ev["metal_redraws"] == 16
    want = pyref.normalize(r)
    assert [x.tobytes() for x in nd] == [x.tobytes() for x in want]
    # a draw that passes ends the loop at once
    draws.clear()
    nd = M.metal_direction(r, n, F(1.0), lambda: (draws.append(1), pyref.v(0.0, 0.5, 0.0))[1])
    assert len(draws) == 1 and pyref.dot(nd, n) > 0


def test_a_mirror_is_unbiased():
    """Rays straight down onto the fuzz-0 mirror floor come back from the light: each result is
    0 (the roulette ended it) or exactly albedo / rr * Le, and the survivors' share is rr."""
    sc = rvcp_amd.scene.specular_cornell_scene()
    cfg = abi.make_config(spp=1)
    lin, trav = mirror()
    mats = sc.aligned_materials()
    floor = mats[sc.mesh.aligned_faces()["material_id"][10]]
    assert int(floor["ty"]) == 1 and float(floor["fuzz"]) == 0.0
    le = [m for m in mats if int(m["ty"]) == 3][0]["albedo"]
    rr = F(cfg["rr_probability"])
    want = np.array([F(F(F(1.0) * F(a / rr)) * l) for a, l in zip(floor["albedo"], le)], F)
    alive = lin.any(axis=1)
    assert np.array_equal(lin[alive].view(np.uint32),
                          np.broadcast_to(want.view(np.uint32), lin[alive].shape))
    assert not lin[~alive].any()
    share = alive.mean()
    sigma = np.sqrt(0.8 * 0.2 / M.MIRROR_N)
    print(f"survivors {int(alive.sum())} of {M.MIRROR_N} = {share:.4f}")
    assert abs(5 * sigma - 0.0625) < 1e-12
    assert abs(share - 0.8) <= 0.0625
    # floor, then the light (survivors) -- or the floor alone
    assert set(np.unique(trav[alive])) == {2} and set(np.unique(trav[~alive])) == {1}


def test_rejected_rays_and_seeds_give_zeros():
    sc, P = paths_ref.scene_of(rvcp_amd.scene.specular_cornell_scene(), abi.make_config(spp=1))
    rays, _ = M.mirror_rays()
    bad = rays[0].copy()
    bad["d"][1] = np.nan
    assert M.radiance(sc, P, bad, F(0.5), 1) == (pyref.v(0, 0, 0), 0)
    assert M.radiance(sc, P, rays[0], F(1.0), 1) == (pyref.v(0, 0, 0), 0)


def test_scene_builder():
    sc = rvcp_amd.scene.specular_cornell_scene(fuzz=0.25, ior=1.3)
    ids = sc.mesh.aligned_faces()["material_id"]
    mats = sc.aligned_materials()
    assert len(mats) == 7 and len(ids) == 32
    assert (mats["ty"][ids[12:22]] == 1).all() and (mats["fuzz"][ids[12:22]] == F(0.25)).all()
    assert (mats["ty"][ids[22:32]] == 2).all()
    assert (mats["refraction_ratio"][ids[22:32]] == F(1.3)).all()
    assert (mats["ty"][ids[10:12]] == 1).all() and (mats["fuzz"][ids[10:12]] == 0).all()
    plain = rvcp_amd.scene.specular_cornell_scene(mirror_floor=False)
    assert (plain.mesh.aligned_faces()["material_id"][10:12] == 0).all()
    assert np.array_equal(sc.luminous_face_ids(), rvcp_amd.Scene.default().luminous_face_ids())
    with pytest.raises(ValueError):
        rvcp_amd.scene.specular_cornell_scene(fuzz=1.5)
