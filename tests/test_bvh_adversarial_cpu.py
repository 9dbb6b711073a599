"""The opt-in BVH's exactness on adversarial input, on the CPU.

tools/bvh4_check.cpp links the product's builder, collapse and quantiser and traces every ray of
tests/bvh_adversarial.py three ways: the brute-force scan, the float-node traversal, and the
traversal over the byte-quantised nodes in the device's own arithmetic (bvh_nearest restated;
IEEE reciprocals where the device has v_rcp_f32 -- tests/test_gpu_bvh_adversarial.py is the
authority for that difference).  Conditions, all judged by bvh_adversarial.evaluate:

  * every mesh is legal input: tree depth and stack bound below kBvhStack;
  * no unexcused disagreement with the scan, for every mesh x ray class x traversal.  Excused:
    only a scan hit whose point (float64) lies outside its face's float box enlarged by the
    builder's own pad (less than half a pad inside counts as outside);
  * excused rays are at most 2 % of any scene's rays, and in camera x interior and
    grazing x interior none whose scan hit is on a well-conditioned face (height at least
    2^-10 of the longest edge; bvh_adversarial.well_conditioned);
  * the ties mesh from within 2 diagonals: no disagreement of any kind, and at least 100 rays
    end on the higher-indexed copy of a duplicated face (every wall of the room is duplicated,
    so any ray that leaves the clutter through a wall ends in a tie: about two rays in three);
  * the same rays with t_min moved onto the hit: the later copy is still found.

Measured (seed 0; 24 108 rays, 41 meshes): excused 16 (float nodes) and 17 (quantised) rays,
0.07 %, the worst scene 0.5 %; all are hits that the exact test reports on sliver or collinear
faces of the fuzz scenes, thousands of pads away from the face.  A ray of any class can pass
such a face on its way (ray seeds 0..7 put 2, 0, 0, 1, 0, 0, 0, 1 of 2296 such hits into the two
zero classes), which is why those classes are conditioned on the face the scan hit, not on
the seed: every seed 0..7 passes.

Planted faults (-DBVH_CHECK_MUTATE, in the model only) that these conditions must notice, each
tried: 1 the cull changed to tn >= bt; 2 the tie rule changed to t < bt; 3 a quantised bound
rounded inward; 4 the box enlargement (pad) taken back to zero; 5 unused child slots kept out
only by their inverted boxes (test_deep_chain_from_afar).  And one fault they found in
the product: bvh4_quantize took the leaf {slot 0, one triangle}, whose reference is ~0, for an
unused child and inverted its box, so the tree's leftmost triangle was never hit (unexcused on
about half of the 36 fuzz scenes before the fix, 146 of 588 rays on one of them).

The model runs with the relative slack of the device's primary-ray traversal (kBvhSlabSlack);
the near-origin rays run again without it, the form of the shadow and path rays (bvh_pool).
Without any slack the far classes fail: from 1000 diagonals 4.3 % (float nodes) and 1.2 %
(quantised) of the vertex-aimed rays were lost, two of them unexcused.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bvh_adversarial as A
import rvcp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc")
MUTATIONS = {1: "cull tn >= bt", 2: "tie rule t < bt", 3: "quantised bound inward", 4: "pad zero"}
CORNELL_FACES = 32


@pytest.fixture(scope="module")
def meshes():
    return A.all_meshes()


@pytest.fixture(scope="module")
def builder_obj(tmp_path_factory):
    """rvcp_bvh.cpp compiled once; every checker variant links it."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    obj = str(tmp_path_factory.mktemp("bvhobj") / "rvcp_bvh.o")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-c",
                    os.path.join(CSRC, "rvcp_bvh.cpp"), "-o", obj], check=True)
    return obj


def _link(obj, exe, *flags):
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, *flags,
                    os.path.join(ROOT, "tools", "bvh4_check.cpp"), obj, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def verdict(builder_obj, meshes, tmp_path_factory):
    d = tmp_path_factory.mktemp("bvhadv")
    exe = _link(builder_obj, str(d / "bvh4_check"))
    return A.evaluate(exe, meshes, str(d))


def test_generator_is_seeded(meshes):
    again = A.all_meshes()
    assert len(meshes) == A.N_FUZZ + 2 + len(A.OFFSET_EXPONENTS)
    for a, b in zip(meshes, again):
        assert a.name == b.name and a.pos.tobytes() == b.pos.tobytes()
        ra, rb = A.make_rays(a, A.RAY_SEED), A.make_rays(b, A.RAY_SEED)
        assert ra[0].tobytes() == rb[0].tobytes()
    rays, tc, oc = A.make_rays(meshes[-1], A.RAY_SEED)
    axis = rays["d"][oc == A.ORIGINS.index("axis")]
    assert np.all(np.count_nonzero(axis, axis=1) == 1) and np.all(np.abs(axis).sum(1) == 1.0)
    ties = [m for m in meshes if m.name == "ties"][0]
    assert ties.upper_duplicates().sum() == 8 + 40          # the walls and the small copies


def test_every_condition_holds(verdict):
    problems, stats = verdict
    print("rays", stats["rays"], "excused", stats["excused"], "ties", stats["ties"])
    for (k, o, t), (n, of) in sorted(stats["shares"].items()):
        print(f"  {k:5s} {o:8s} x {t:8s}: {n} of {of} excused ({100.0 * n / of:.2f} %)")
    print("  worst scene share", max(stats["per_scene"].values()))
    assert not problems, f"{len(problems)} violated conditions, first: " + "; ".join(problems[:5])
    assert stats["rays"] > 20000 and stats["ties"] >= A.MIN_TIES


@pytest.mark.parametrize("k", sorted(MUTATIONS))
def test_planted_fault_is_noticed(builder_obj, meshes, tmp_path, k):
    exe = _link(builder_obj, str(tmp_path / f"bvh4_mut{k}"), f"-DBVH_CHECK_MUTATE={k}")
    some = [m for m in meshes if not m.name.startswith("fuzz")] + meshes[:6]
    problems, _ = A.evaluate(exe, some, str(tmp_path))
    assert problems, f"the suite accepts a model with the fault '{MUTATIONS[k]}'"


@pytest.mark.parametrize("ratio", [1.3, 1.5])
def test_deep_chain_from_afar(builder_obj, tmp_path, ratio):
    """A tree as deep as the stack allows (stack bound exactly kBvhStack) holding a node a few
    pads wide, seen from 100 / 300 / 1000 diagonals: the checker fails if either traversal's
    stack passes bvh4_collapse's bound.  From there an unused slot's inverted box no longer
    keeps a ray out (fma(255, a, b) == b); only its reference does.  The model with that left
    out (fault 5) must overrun the bound, and the real one must not, with no unexcused ray."""
    m = A.chain_mesh(ratio)
    rays = A.far_rays(m)
    exe = _link(builder_obj, str(tmp_path / "bvh4_check"))
    res, info, p = A.run_checker(exe, m, rays, str(tmp_path))
    assert info["depth"] < A.stack_entries() and info["stack"] == A.stack_entries(), info
    assert res is not None, p.stdout + p.stderr
    for k in ("float", "quant"):
        _, why = A.classify(m, rays, res["brute"], res[k], info["pad_abs"])
        assert not why, (k, why[:3])
    assert (res["brute"]["face"] >= 0).sum() >= 300
    bad = _link(builder_obj, str(tmp_path / "bvh4_mut5"), "-DBVH_CHECK_MUTATE=5")
    res, info, p = A.run_checker(bad, m, rays, str(tmp_path))
    assert res is None and p.returncode == 1, "the model enters unused slots and stays within the stack bound"
    deepest = int([l for l in p.stdout.splitlines() if l.startswith("rays")][0].split()[-1])
    assert deepest > A.stack_entries(), p.stdout


def test_hybrid_prefix_ties_in_the_model(builder_obj, tmp_path):
    """The checker's `hybrid` rays mode on the GPU suite's hybrid scene: Cornell's 32 faces
    stay out of the tree (bvh_big_prefix), the ties mesh and copies of the twelve room faces are
    in it, and a copy in the tree at equal t beats its prefix original.  No disagreement."""
    cornell = rvcp_amd.Scene.default()
    v = cornell.mesh.aligned_vertices()["position"][:, :3]
    cpos = v[cornell.mesh.aligned_faces()["vertices"]].astype(np.float32)
    ties = A.ties_mesh()
    pos = np.concatenate([cpos, (ties.pos + np.float32([0, 274, 0])).astype(np.float32), cpos[:12]])
    m = A.Mesh("hybrid", pos, np.zeros(len(pos)), cornell.camera.position, [0, 274, 0], 1e-4, t_near=0.1)
    rays = A.primary_rays(cornell.camera, 47, 39)
    exe = _link(builder_obj, str(tmp_path / "bvh4_check"))
    for noslack in (False, True):
        res, info, p = A.run_checker(exe, m, rays, str(tmp_path), hybrid=True, noslack=noslack)
        assert res is not None, p.stdout + p.stderr
        assert info["prefix"] == CORNELL_FACES == len(cpos)
        for k in ("float", "quant"):
            assert np.array_equal(res[k], res["brute"]), (k, noslack)
        f = res["brute"]["face"][res["brute"]["face"] >= 0]
        assert (f >= len(pos) - 12).sum() >= 100 and not (f < 12).any()


def test_gpu_cameras_in_the_model(builder_obj, meshes, tmp_path):
    """The cameras of tests/test_gpu_bvh_adversarial.py, their primary rays restated in float32
    numpy, through the model: every frame of a well-formed mesh sees it and agrees with the
    scan on every pixel; on the fuzz scenes no unexcused pixel."""
    exe = _link(builder_obj, str(tmp_path / "bvh4_check"))
    for m in [m for m in meshes if not m.name.startswith("fuzz")] + meshes[:4]:
        cams = A.gpu_cameras(m)
        assert cams[0][0] == "camera"
        for kind, cam in cams:
            rays = A.primary_rays(cam, 47, 39)
            res, info, p = A.run_checker(exe, m, rays, str(tmp_path))
            assert res is not None, p.stdout + p.stderr
            for k in ("float", "quant"):
                c, why = A.classify(m, rays, res["brute"], res[k], info["pad_abs"])
                assert not why, (m.name, kind, k, why[:3])
                if not m.name.startswith("fuzz"):
                    assert not c.any(), (m.name, kind, k, int(np.count_nonzero(c)))
                    assert (res["brute"]["face"] >= 0).sum() >= 50, (m.name, kind)


def test_model_under_sanitizers(meshes, verdict, tmp_path):
    """The stand-alone checker with the builder under AddressSanitizer / UBSan (host code,
    nothing preloaded): no report, and every condition holds as in the plain build."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("sanitizer runtime unavailable: " + r.stderr[-200:])
    exe = str(tmp_path / "bvh4_asan")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *san,
                        "-I", CSRC, os.path.join(ROOT, "tools", "bvh4_check.cpp"),
                        os.path.join(CSRC, "rvcp_bvh.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    some = [m for m in meshes if not m.name.startswith("fuzz")] + meshes[:8]
    for m in some:
        rays, _, _ = A.make_rays(m, A.RAY_SEED)
        _, _, p = A.run_checker(exe, m, rays, str(tmp_path))
        assert p.returncode == 0, (m.name, p.stdout[-500:], p.stderr[-2000:])
        assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
    problems, _ = A.evaluate(exe, some, str(tmp_path))
    assert not problems, problems[:5]
