"""Every kernel schedule on every adversarial input, against the CPU oracle.

include/rvcp.h promises that every schedule renders bit-identical frames, and the host sends
the most demanding workloads to schedules 5, 10 and 6.  Their pretest gates, their two
triangles per step, the tail form's merges, the shadow stop and schedule 6's specialised scan
are arguments about magnitude, rounding and the order of equal hits; so the inputs written to
attack exactly those -- the fuzz scenes of tests/fuzz_scenes.py, the tie, offset and degenerate
meshes of tests/bvh_adversarial.py and the tile-seam stacks of tests/tile_ties.py -- are forced
through each schedule here and compared with the oracle, with the project's own tolerance:

    linear RGB bits equal, RGBA8 bytes equal, `traversals` equal; nothing excused.

Every case also asserts that the schedule asked for is the one that ran (with the
VARIANT_SPECIALIZED bit where the case is the specialised module) and that the frame is not
empty (more traversals than samples).  tests/test_tile_ties_cpu.py holds the conditions on the
inputs: that a wrong tie winner in any stack changes at least 10 pixels of these very frames.

Frame sizes.  The host spreads a small frame over up to two waves per SIMD, 8 pixels a wave
(static_split), and a wave with 32 rays or fewer scans in the tail form: R lanes per ray, the
exact test alone, merged by the tie rule.  So the 48 x 40, 47 x 39 and 9 x 7 frames reach the
tail forms and their merges in every schedule -- and nothing else of the tiled scans.  The
steps of two triangles, "the last triangles of a tile", the pretest gates and the shadow stop
run only in waves that start with more than 32 rays; the *_full_waves tests render the same
scenes at 416 x 320 and 376 x 312 for them (about a second of the oracle each).  Tried in
scratch builds: with the tail merges' tie rule cut to `ot < bt` every tie-mesh test but that of
`degenerate` (one material in its run) fails, at schedules 3, 4, 5 and 10 and at every size;
with the `+ h` dropped from `best = base + i + h` only the *_full_waves tests fail (schedules
4, 5 and 10), the small frames all pass.

The G-buffer tests compare the brute-force G-buffer kernel, the reference of every BVH
G-buffer test, with denoise_ref.cpu_gbuffer byte for byte."""
import functools

import numpy as np
import pytest

import bvh_adversarial as A
import denoise_ref as R
import oracle as O
import rvcp_amd
import tile_ties as T
from conftest import scene_arrays
from fuzz_scenes import N_FUZZ, _with_specks, fuzz_scene
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
SPEC = abi.VARIANT_SPECIALIZED
OFF = abi.SPECIALIZE_OFF
FW, FH = 48, 40                     # the fuzz scenes' frame (test_gpu_spec_fuzz.py)
FUZZ_BIG = (416, 320)               # 64 pixels for each of 2080 waves: full waves from the start
W, H = T.W, T.H                     # the tie meshes' frame: 47 x 39
SMALL = (9, 7)                      # one partly filled wave
TIME = 3.0


def _gpu(sc, w, h, t, **kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(sc)
        rgba, lin = rt.render(w, h, t, want_linear=True)
        return rgba, lin, rt.last_stats.copy()


def _compare(problems, label, got, orc, variant, spec, samples):
    """Append to `problems` what the frame `got` = (rgba, linear, stats) misses: the schedule
    that ran, a frame that is not empty, equality with the oracle's (linear, rgba, traversals)."""
    rgba, lin, stats = got
    o_lin, o_rgba, o_trav = orc
    kv = int(stats["kernel_variant"])
    if kv & 15 != variant or bool(kv & SPEC) != spec:
        problems.append(f"{label}: kernel_variant {kv}, wanted schedule {variant}, specialised {spec}")
    if not int(o_trav) > samples:
        problems.append(f"{label}: an empty frame, {o_trav} traversals of {samples} samples")
    diff = np.any(lin.view(np.uint32) != o_lin.view(np.uint32), axis=-1)
    if diff.any():
        problems.append(f"{label}: {int(diff.sum())} pixels differ in linear RGB, first at "
                        f"{np.argwhere(diff)[:3].tolist()}")
    if not np.array_equal(rgba, o_rgba):
        problems.append(f"{label}: {int(np.any(rgba != o_rgba, axis=-1).sum())} pixels differ in RGBA8")
    if int(stats["traversals"]) != int(o_trav):
        problems.append(f"{label}: traversals {int(stats['traversals'])}, the oracle's {int(o_trav)}")


# ------------------------------------------------------------------------------ fuzz scenes
@functools.lru_cache(maxsize=None)
def _fuzz(seed, specks=0, w=FW, h=FH):
    """(scene, config kwargs, description, the oracle's frame), the oracle rendered once."""
    sc, kw, desc = fuzz_scene(seed)
    if specks:
        sc = _with_specks(sc, specks, seed)
        desc += f", {specks} specks: {len(sc.mesh.aligned_faces())} faces"
    orc = O.render(scene_arrays(sc), sc.push_constant(100.0 + seed), abi.make_config(**kw), w, h)
    for a in orc[:2]:
        a.setflags(write=False)
    return sc, kw, desc, orc


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_every_schedule(seed):
    """Schedules 1, 2, 4, 5, 6 and 10 with the generic scan and schedule 6 with the
    scene-specialised module (jk->path6, what the headline runs) on every fuzz scene.  Schedule 3,
    generic and specialised, is test_gpu_spec_fuzz.py's."""
    sc, kw, desc, orc = _fuzz(seed)
    problems = []
    for v in (1, 2, 4, 5, 6, 10):
        got = _gpu(sc, FW, FH, 100.0 + seed, kernel_variant=v, specialize=OFF, **kw)
        _compare(problems, f"schedule {v} generic", got, orc, v, False, FW * FH * kw["spp"])
    got = _gpu(sc, FW, FH, 100.0 + seed, kernel_variant=6, **kw)
    _compare(problems, "schedule 6 specialised", got, orc, 6, True, FW * FH * kw["spp"])
    assert not problems, f"{problems}; {desc}"


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_tiled_across_tile_boundary(seed):
    """The tiled schedules on every fuzz scene with 230 small triangles appended: slivers,
    2^38 offsets and 2^-20 rooms over a tile boundary.  Where 230 leaves a scene within one
    tile, nearly full, it runs again with 240 (tile_ties.speck_counts)."""
    sc0 = fuzz_scene(seed)[0]
    problems = []
    for n in T.speck_counts(sc0):
        sc, kw, desc, orc = _fuzz(seed, n)
        for v in (4, 5, 10):
            got = _gpu(sc, FW, FH, 100.0 + seed, kernel_variant=v, specialize=OFF, **kw)
            _compare(problems, f"{n} specks, schedule {v}", got, orc, v, False, FW * FH * kw["spp"])
    n_faces = len(sc.mesh.aligned_faces())
    assert T.TILE < n_faces <= 2 * T.TILE, desc
    assert not problems, f"{problems}; {desc}"


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_tiled_full_waves(seed):
    """The same scenes, across the tile boundary, at 416 x 320.  A 48 x 40 frame is spread over
    waves of 8 pixels (static_split), which scan in the tail form -- the exact test alone --
    from their first iteration; only a frame that gives a wave more than 32 rays runs the
    steps of two triangles and with them the pretest gates (tri_stage1a, tri_maybe_a,
    |n2| <= m) and the shadow stop.  This is the case that sends the slivers, the 2^38 offsets
    and the 2^-20 rooms through the gates; the oracle needs about a second for it."""
    sc0 = fuzz_scene(seed)[0]
    sc, kw, desc, orc = _fuzz(seed, T.speck_counts(sc0)[-1], *FUZZ_BIG)
    assert T.TILE < len(sc.mesh.aligned_faces()) <= 2 * T.TILE, desc
    problems = []
    for v in (4, 5, 10):
        got = _gpu(sc, *FUZZ_BIG, 100.0 + seed, kernel_variant=v, specialize=OFF, **kw)
        _compare(problems, f"schedule {v}", got, orc, v, False, FUZZ_BIG[0] * FUZZ_BIG[1] * kw["spp"])
    assert not problems, f"{problems}; {desc}"


# ------------------------------------------------------------------------------- tie meshes
TIE_MESHES = (["ties"] + [f"offset2^{e}" for e in A.OFFSET_EXPONENTS] + ["degenerate", "degenerate_alt"] +
              [f"tile_ties{n}" for n in sorted(T.STACKS)])


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "ties":
        return A.ties_mesh()
    if name == "degenerate":
        return A.degenerate_mesh()
    if name == "degenerate_alt":
        return T.degenerate_alternating_mesh()
    if name.startswith("tile_ties"):
        return T.tile_ties_mesh(int(name[9:]))
    return A.offset_mesh(int(name.split("^")[1]))


@functools.lru_cache(maxsize=None)
def _tie_oracle(name, w, h, t=TIME):
    orc = T.oracle_frame(_mesh(name), t, w, h)
    for a in orc[:2]:
        a.setflags(write=False)
    return orc


def _tie_schedules(name, w, h, schedules=((3, 3), (4, 4), (5, 5), (10, 10), (0, 5))):
    mesh = _mesh(name)
    sc, kw = mesh.scene(), T.path_config(mesh)
    orc = _tie_oracle(name, w, h)
    problems = []
    # schedule 0: the host's own choice, which for 256 or more faces on a small frame is 5
    assert len(mesh.pos) >= 256
    for asked, v in schedules:
        got = _gpu(sc, w, h, TIME, kernel_variant=asked, specialize=OFF, **kw)
        _compare(problems, f"schedule {asked}", got, orc, v, False, w * h * kw["spp"])
    assert not problems, f"{name} at {w} x {h}: {problems}"


@pytest.mark.parametrize("name", TIE_MESHES)
def test_tie_meshes_every_schedule(name):
    """Exact ties in t -- duplicated faces before and after their originals, coplanar pairs,
    200 identical faces, stacks at the tiles' seams -- through the generic scan (3), the tiled
    scans (4, 5), the tiled scan with the ray pool (10) and the automatic choice."""
    _tie_schedules(name, W, H)


@pytest.mark.parametrize("name", ["ties"] + [f"tile_ties{n}" for n in sorted(T.STACKS)])
def test_tie_meshes_one_partial_wave(name):
    """9 x 7: the whole frame is one partly filled wave, so the scan's tail form takes over
    early and schedule 10's pool holds fewer rays than a pass."""
    _tie_schedules(name, *SMALL)


@pytest.mark.parametrize("name", ["ties", "degenerate_alt"] + [f"tile_ties{n}" for n in sorted(T.STACKS)])
def test_tie_meshes_full_waves(name):
    """376 x 312, the same cameras: the host spreads the small frames above over so many waves
    (8 pixels each, static_split) that every wave scans in the tail form from its first
    iteration, and a scratch build whose two-triangle step names the wrong face of its pair
    passes them all.  Here a wave starts with 58 pixels or more, above the 32 rays at which the
    tail form and the pool's take over, so the tiled scans run their steps of two triangles
    and "the last triangles of a tile"; the oracle needs about a second for such a frame."""
    _tie_schedules(name, T.BIG_SCALE * W, T.BIG_SCALE * H, schedules=((4, 4), (5, 5), (10, 10)))


# ---------------------------------------------------------------------------------- batches
BATCH_TIMES = (3.0, 7.5, 301.25)


@pytest.mark.parametrize("variant", [3, 4, 5, 10])
def test_tile_ties_batch(variant):
    """rvcp_render_frames_async: three frames of three times in one path kernel, each equal
    to the oracle's frame of its own time (the call as in test_gpu_batch.py)."""
    import torch
    name = f"tile_ties{T.SMALL}"
    mesh = _mesh(name)
    sc, kw = mesh.scene(), T.path_config(mesh)
    n = len(BATCH_TIMES)
    with rvcp_amd.RayTracer(kernel_variant=variant, specialize=OFF, **kw) as rt:
        rt.upload_scene(sc)
        out = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
        lin = torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda")
        rt.render_frames_async([sc.push_constant(t) for t in BATCH_TIMES], W, H, 0, 1,
                               out.data_ptr(), lin.data_ptr())
        st = rt.sync_stats()
        torch.cuda.synchronize()
    out, lin = out.cpu().numpy().view(np.uint8).reshape(n, H, W, 4), lin.cpu().numpy()
    orcs = [_tie_oracle(name, W, H, t) for t in BATCH_TIMES]
    kv = int(st["kernel_variant"])
    assert kv & 15 == variant and not kv & SPEC, kv
    for f, (o_lin, o_rgba, o_trav) in enumerate(orcs):
        assert int(o_trav) > W * H * kw["spp"], f
        diff = np.any(lin[f].view(np.uint32) != o_lin.view(np.uint32), axis=-1)
        assert not diff.any(), f"frame {f}: {int(diff.sum())} pixels differ, first at {np.argwhere(diff)[:3].tolist()}"
        assert np.array_equal(out[f], o_rgba), f
    assert not np.array_equal(orcs[0][1], orcs[1][1])           # the seeds differ
    assert int(st["traversals"]) == sum(int(o[2]) for o in orcs)


# --------------------------------------------------------------------------------- G-buffer
GW, GH = 24, 20
GBUFFER_SEEDS = T.GBUFFER_SEEDS      # every frame holds both hits and misses, asserted below


def _gbuffer_scene(name):
    if name.startswith("fuzz"):
        return fuzz_scene(int(name[4:]))[0]
    # the small tile-ties mesh, its first 96 faces (the room, two stacks and filler): the
    # pure-Python scan of all 513 takes 9 s
    m = _mesh(f"tile_ties{T.SMALL}")
    sub = A.Mesh("tile_ties_head", m.pos[:96], m.mats[:96], m.cam_pos, m.look, m.t_min, t_near=m.t_near)
    return sub.scene(m.camera())


@functools.lru_cache(maxsize=None)
def _cpu_gbuffer(name):
    g = R.cpu_gbuffer(_gbuffer_scene(name), GW, GH)
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("name", [f"fuzz{s}" for s in GBUFFER_SEEDS] + ["tile_ties_head"])
def test_gbuffer_brute_force_equals_cpu_scan(name):
    import torch
    sc = _gbuffer_scene(name)
    ref = _cpu_gbuffer(name)
    miss = ref["face"] == R.MISS
    assert miss.any() and not miss.all(), f"{name}: {int(miss.sum())} misses of {miss.size} texels"
    if name.startswith("fuzz"):
        desc = fuzz_scene(int(name[4:]))[2]
    else:
        desc = name
        won = np.unique(ref["face"][~miss])
        assert {23, 44} <= set(won.tolist()) and not set(won.tolist()) & {20, 21, 22, 41, 42, 43}
    with rvcp_amd.RayTracer(spp=1, specialize=OFF, accel=abi.ACCEL_NONE) as rt:
        rt.upload_scene(sc)
        buf = torch.zeros(GW * GH * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rt.render_gbuffer_async(sc.push_constant(0.0), GW, GH, buf.data_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(GH, GW)
    bad = np.argwhere((got.view(np.uint8).reshape(GH, GW, 32) != ref.view(np.uint8).reshape(GH, GW, 32)).any(-1))
    assert not len(bad), (f"{len(bad)} texels differ, first {bad[0].tolist()}: {got[tuple(bad[0])]} != "
                          f"{ref[tuple(bad[0])]}; {desc}")
