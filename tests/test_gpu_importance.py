"""Cosine-weighted bounce sampling on the GPU (rvcp_set_sampling).

The mode has no C oracle, so exactness is checked in three steps: schedule 1 with the generic
scan equals the committed frames of the pure-Python restatement (tests/importance_ref.py,
tests/golden/importance_frames.npz) bit for bit; every other path the games101 integrator can
take -- schedules 2 to 6 and 10, the scene-specialised modules, the BVH path kernel and the
hybrid, batches and shards -- equals schedule 1 bit for bit in cosine mode, on the adversarial
scenes and at the frame sizes of test_gpu_schedules_adversarial; and with max_bounces = 1, where
the bounce is drawn and never used, cosine frames equal the C oracle's.  Tolerance throughout:
linear RGB bits, RGBA8 bytes and the traversal count equal, nothing excused.

The default mode must be what it was: switching to cosine and back leaves frames equal to the
oracle.  Two statistical tests say that the new estimator is a correct and a better one: on a
closed box, where the shader's unattenuated miss term cannot act, the two modes converge to the
same image within the uniform mode's own noise, and a cosine frame is closer to its own
converged mean than a uniform frame is to its."""
import os

import numpy as np
import pytest

import importance_ref as I
import oracle as O
import rvcp_amd
import tile_ties as T
from conftest import ROOT, scene_arrays
from fuzz_scenes import _with_specks, fuzz_scene
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
SPEC = abi.VARIANT_SPECIALIZED
OFF = abi.SPECIALIZE_OFF
UNI, COS = abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE
FIXTURE = os.path.join(ROOT, "tests", "golden", "importance_frames.npz")
SIZES = [(9, 7), (48, 40), (416, 320)]   # one partly filled wave, tail forms, full waves
FUZZ_SEEDS = (2, 3, 5, 11)               # scale 1; 2^22 moved by 2^38; 2^10 moved by 2^24; 2^16
HYBRID_SPECKS = 160                      # test_gpu_spec_fuzz.test_bvh_hybrid_fuzz's count


def _gpu(sc, w, h, t, sampling=COS, **kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.sampling = sampling
        rt.upload_scene(sc)
        rgba, lin = rt.render(w, h, t, want_linear=True)
        assert rt.sampling == sampling
        return rgba, lin, rt.last_stats.copy()


def _same(problems, label, got, ref, variant=None, spec=None):
    rgba, lin, stats = got
    r_rgba, r_lin, r_trav = ref
    kv = int(stats["kernel_variant"])
    if variant is not None and (kv & 15 != variant or (spec is not None and bool(kv & SPEC) != spec)):
        problems.append(f"{label}: kernel_variant {kv}, wanted schedule {variant}, specialised {spec}")
    diff = np.any(lin.view(np.uint32) != r_lin.view(np.uint32), axis=-1)
    if diff.any():
        problems.append(f"{label}: {int(diff.sum())} pixels differ in linear RGB, first at "
                        f"{np.argwhere(diff)[:3].tolist()}")
    if not np.array_equal(rgba, r_rgba):
        problems.append(f"{label}: {int(np.any(rgba != r_rgba, axis=-1).sum())} pixels differ in RGBA8")
    if int(stats["traversals"]) != int(r_trav):
        problems.append(f"{label}: traversals {int(stats['traversals'])}, wanted {int(r_trav)}")


# ------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("case", list(I.CASES))
def test_schedule_1_equals_the_restatement(case):
    d = np.load(FIXTURE)
    sc, kw, W, H = I.case_scene(case)
    got = _gpu(sc, W, H, I.FIXTURE_TIME, kernel_variant=1, specialize=OFF, **kw)
    problems = []
    _same(problems, case, got, (d[case + "/rgba"], d[case + "/linear"], d[case + "/traversals"]), 1, False)
    assert not problems, problems


# ------------------------------------------------------------------------- schedule agreement
def _agreement(sc, sc_specks, kw, w, h, t, small_scene):
    """Every path against schedule 1 (generic), all in cosine mode; `small_scene`: at most 64
    faces, so that the specialised modules exist.  Returns (problems, hybrid engaged)."""
    ref = _gpu(sc, w, h, t, kernel_variant=1, specialize=OFF, **kw)
    ref = (ref[0], ref[1], int(ref[2]["traversals"]))
    assert ref[2] > w * h * kw["spp"], "an empty frame"
    problems = []
    for v in (2, 3, 4, 5, 6, 10):
        _same(problems, f"schedule {v} generic",
              _gpu(sc, w, h, t, kernel_variant=v, specialize=OFF, **kw), ref, v, False)
    if small_scene:
        for v in (3, 6):
            _same(problems, f"schedule {v} specialised",
                  _gpu(sc, w, h, t, kernel_variant=v, **kw), ref, v, True)
    _same(problems, "BVH path kernel",
          _gpu(sc, w, h, t, accel=abi.ACCEL_BVH, specialize=OFF, **kw), ref, 7, False)
    # the hybrid: leading big faces by the specialised scan, the BVH over the rest
    ref2 = _gpu(sc_specks, w, h, t, kernel_variant=1, specialize=OFF, **kw)
    ref2 = (ref2[0], ref2[1], int(ref2[2]["traversals"]))
    hyb = _gpu(sc_specks, w, h, t, accel=abi.ACCEL_BVH, **kw)
    _same(problems, "BVH hybrid", hyb, ref2, 7)
    return problems, bool(int(hyb[2]["kernel_variant"]) & SPEC)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_every_schedule_agrees_fuzz(seed, w, h):
    sc, kw, desc = fuzz_scene(seed)
    problems, engaged = _agreement(sc, _with_specks(sc, HYBRID_SPECKS, seed), kw, w, h,
                                   100.0 + seed, True)
    assert not problems, f"{problems}; {desc}"
    print(f"seed {seed} {w}x{h}: hybrid engaged {engaged}")


def test_the_hybrid_engages_in_cosine_mode():
    engaged = 0
    for seed in FUZZ_SEEDS:
        sc, kw, _ = fuzz_scene(seed)
        st = _gpu(_with_specks(sc, HYBRID_SPECKS, seed), 9, 7, 1.0, accel=abi.ACCEL_BVH, **kw)[2]
        engaged += bool(int(st["kernel_variant"]) & SPEC)
    assert engaged == len(FUZZ_SEEDS), f"the hybrid's cosine module ran on {engaged} of {len(FUZZ_SEEDS)} scenes"


@pytest.mark.parametrize("w,h", SIZES)
def test_every_schedule_agrees_tie_mesh(w, h):
    mesh = T.tile_ties_mesh(T.SMALL)
    sc, kw = mesh.scene(), T.path_config(mesh)
    problems, _ = _agreement(sc, sc, kw, w, h, 3.0, False)
    assert not problems, problems


# --------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("seed", FUZZ_SEEDS[:2])
def test_one_bounce_equals_the_oracle(seed):
    """max_bounces = 1: the bounce is drawn (the rand() stream advances as ever) and never
    traced, and its weight never multiplies a contribution: cosine frames are the oracle's."""
    sc, kw, desc = fuzz_scene(seed)
    kw = dict(kw, max_bounces=1)
    t = 100.0 + seed
    o_lin, o_rgba, o_trav = O.render(scene_arrays(sc), sc.push_constant(t), abi.make_config(**kw), 48, 40)
    problems = []
    for label, v, extra, spec in (("schedule 1", 1, dict(specialize=OFF), False),
                                  ("schedule 6 specialised", 6, {}, True),
                                  ("schedule 10", 10, dict(specialize=OFF), False)):
        _same(problems, label, _gpu(sc, 48, 40, t, kernel_variant=v, **extra, **kw),
              (o_rgba, o_lin, o_trav), v, spec)
    assert not problems, f"{problems}; {desc}"


# ----------------------------------------------------------------------------- the switch
def test_default_mode_is_untouched_and_the_switch_behaves(cornell, cornell_arrays):
    W, H, t = 48, 40, 123.0
    o_lin, o_rgba, o_trav = O.render(cornell_arrays, cornell.push_constant(t), abi.make_config(spp=3), W, H)
    for kw in (dict(), dict(specialize=OFF), dict(kernel_variant=1)):
        with rvcp_amd.RayTracer(spp=3, **kw) as rt:
            L, h = rt._lib, rt.handle
            assert rt.sampling == UNI
            rt.upload_scene(cornell)
            rt.sampling = COS
            assert rt.sampling == COS
            c_rgba, c_lin = rt.render(W, H, t, want_linear=True)
            c_trav = int(rt.last_stats["traversals"])
            rt.upload_scene(cornell)                    # the switch survives a re-upload
            assert rt.sampling == COS
            c2 = rt.render(W, H, t, want_linear=True)
            assert np.array_equal(c2[1].view(np.uint32), c_lin.view(np.uint32))
            assert int(rt.last_stats["traversals"]) == c_trav
            # unknown values, and a frame in flight
            for bad in (2, -1, 77):
                assert L.rvcp_set_sampling(h, bad) == abi.RVCP_E_INVALID
            assert L.rvcp_get_sampling(h, None) == abi.RVCP_E_INVALID
            assert rt.sampling == COS
            rt.sampling = COS                           # the value it has: nothing happens
            rt.sampling = UNI
            assert rt.sampling == UNI
            rgba, lin = rt.render(W, H, t, want_linear=True)
            assert np.array_equal(lin.view(np.uint32), o_lin.view(np.uint32)), kw
            assert np.array_equal(rgba, o_rgba) and int(rt.last_stats["traversals"]) == int(o_trav)
            # the cosine frame is another image of the same scene
            assert not np.array_equal(c_lin.view(np.uint32), o_lin.view(np.uint32))
            assert np.isfinite(c_lin).all() and abs(float(c_lin.mean()) / float(o_lin.mean()) - 1) < 0.25


def test_set_sampling_with_a_frame_in_flight(cornell):
    torch = pytest.importorskip("torch")
    out = torch.zeros((64, 64), dtype=torch.int32, device="cuda")
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        rt.render_async(cornell.push_constant(1.0), 64, 64, out.data_ptr())
        assert rt._lib.rvcp_set_sampling(rt.handle, COS) == abi.RVCP_E_INVALID     # as rvcp_set_taa
        assert rt.sampling == UNI
        rt.wait()
        rt.sampling = COS
        torch.cuda.synchronize()


def test_legacy_context_refuses_cosine(cornell):
    with rvcp_amd.RayTracer(integrator=abi.INTEGRATOR_LEGACY) as rt:
        assert rt._lib.rvcp_set_sampling(rt.handle, COS) == abi.RVCP_E_UNSUPPORTED
        assert rt._lib.rvcp_set_sampling(rt.handle, 5) == abi.RVCP_E_INVALID
        rt.sampling = UNI
        assert rt.sampling == UNI


# ------------------------------------------------------------------------- batches and shards
@pytest.mark.parametrize("kw", [dict(), dict(kernel_variant=10), dict(kernel_variant=3, specialize=OFF)])
def test_batch_equals_single_frames(cornell, kw):
    torch = pytest.importorskip("torch")
    W, H, times = 47, 39, (3.0, 7.5)
    with rvcp_amd.RayTracer(spp=3, **kw) as rt:
        rt.sampling = COS
        rt.upload_scene(cornell)
        singles = []
        for t in times:
            rgba, lin = rt.render(W, H, t, want_linear=True)
            singles.append((rgba, lin, int(rt.last_stats["traversals"])))
        out = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
        lin = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")
        rt.render_frames_async([cornell.push_constant(t) for t in times], W, H, 0, 1,
                               out.data_ptr(), lin.data_ptr())
        st = rt.sync_stats()
        torch.cuda.synchronize()
    out = out.cpu().numpy().view(np.uint8).reshape(2, H, W, 4)
    lin = lin.cpu().numpy()
    for f, (s_rgba, s_lin, _) in enumerate(singles):
        assert np.array_equal(lin[f].view(np.uint32), s_lin.view(np.uint32)), f
        assert np.array_equal(out[f], s_rgba), f
    assert int(st["traversals"]) == sum(s[2] for s in singles)
    assert not np.array_equal(singles[0][0], singles[1][0])


def test_two_shards_assemble_to_the_whole_frame(cornell):
    torch = pytest.importorskip("torch")
    W, H, t, n = 47, 39, 5.0, 2
    with rvcp_amd.RayTracer(spp=3) as rt:
        rt.sampling = COS
        rt.upload_scene(cornell)
        whole = rt.render(W, H, t, want_linear=True)[1]
        shards = []
        for k in range(n):
            rows = rvcp_amd.shard_rows(H, k, n)
            out = torch.zeros((rows, W), dtype=torch.int32, device="cuda")
            lin = torch.zeros((rows, W, 3), dtype=torch.float32, device="cuda")
            rt.render_shard_async(cornell.push_constant(t), W, H, k, n, out.data_ptr(), lin.data_ptr())
            rt.sync_stats()
            torch.cuda.synchronize()
            shards.append(lin.cpu().numpy())
    frame = np.zeros_like(whole)
    for y in range(H):                   # stripes of 8 rows go round the shards (rvcp_shard_rows)
        stripe = y >> 3
        frame[y] = shards[stripe % n][(stripe // n) * 8 + (y & 7)]
    assert np.array_equal(frame.view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("n_gpus", [2, 3])
def test_sub_contexts_take_the_mode(cornell, n_gpus):
    """n_gpus > 1 (the sub-contexts share the device where there is one GPU): the frame the
    context assembles from its shards is the one-context frame, in cosine mode and after the
    switch back; set before and after the upload."""
    W, H, t = 47, 39, 5.0
    one_c = _gpu(cornell, W, H, t, spp=3)
    one_u = _gpu(cornell, W, H, t, sampling=UNI, spp=3)
    with rvcp_amd.RayTracer(spp=3, n_gpus=n_gpus) as rt:
        rt.sampling = COS
        rt.upload_scene(cornell)
        rgba, lin = rt.render(W, H, t, want_linear=True)
        assert np.array_equal(lin.view(np.uint32), one_c[1].view(np.uint32))
        assert np.array_equal(rgba, one_c[0])
        rt.sampling = UNI
        rgba, lin = rt.render(W, H, t, want_linear=True)
        assert np.array_equal(lin.view(np.uint32), one_u[1].view(np.uint32))
        rt.sampling = COS
        assert np.array_equal(rt.render(W, H, t), one_c[0])


# ------------------------------------------------- the chains on top, the loop, the C example
def test_chains_run_on_top_and_the_switch_drops_their_histories(cornell):
    W = H = 48
    with rvcp_amd.RayTracer(spp=3) as rt:
        rt.upload_scene(cornell)
        rt.sampling = COS
        raw = rt.render(W, H, 1.0, want_linear=True)[1]
        den = rt.render_denoised(W, H, 1.0, want_linear=True)[1]
        assert np.isfinite(den).all() and abs(float(den.mean()) / float(raw.mean()) - 1) < 0.2
        t1 = rt.render_temporal(W, H, 1.0, want_linear=True, want_history=True)
        t2 = rt.render_temporal(W, H, 2.0, want_linear=True, want_history=True)
        s1 = rt.render_svgf(W, H, 1.0, want_linear=True, want_history=True)
        s2 = rt.render_svgf(W, H, 2.0, want_linear=True, want_history=True)
        for a, b in ((t1, t2), (s1, s2)):
            assert np.isfinite(b[1]).all()
            assert int(b[2].max()) == int(a[2].max()) + 1           # the history grew
        # the first accumulated frame is the cosine frame itself
        assert np.array_equal(t1[1].view(np.uint32), raw.view(np.uint32))
        rt.sampling = COS                                           # no change: histories stay
        assert int(rt.render_temporal(W, H, 3.0, want_history=True)[1].max()) == int(t2[2].max()) + 1
        rt.sampling = UNI                                           # a change: both restart
        t4 = rt.render_temporal(W, H, 4.0, want_history=True)
        s4 = rt.render_svgf(W, H, 4.0, want_history=True)
        assert int(t4[1].max()) == int(t1[2].max()) and int(s4[1].max()) == int(s1[2].max())


def test_headless_loop_passes_the_mode_through(cornell):
    from rvcp_amd import interactive
    sc = rvcp_amd.Scene.default()
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(sc)
        want = {}
        for mode in (COS, UNI):
            rt.sampling = mode
            want[mode] = rt.render(32, 24, 1.0)
        seen = []
        for mode in (COS, UNI):
            interactive.run_headless(rt, sc, 2, 32, 24, fixed_dt=0.0, time_seed=lambda i: float(i),
                                     on_fps=lambda n: None, sampling=mode)
            assert rt.sampling == mode
            seen.append(rt.render(32, 24, 1.0))
        interactive.run_headless(rt, sc, 1, 32, 24, fixed_dt=0.0, time_seed=lambda i: 0.0,
                                 on_fps=lambda n: None)                  # None: the mode stays
        assert rt.sampling == UNI
    assert np.array_equal(seen[0], want[COS]) and np.array_equal(seen[1], want[UNI])
    assert not np.array_equal(want[COS], want[UNI])


def test_c_example_flag(tmp_path, cornell):
    import subprocess
    exe = os.path.join(ROOT, "examples", "build", "rvcp_render")
    scene = str(tmp_path / "s.rvcpscn")
    rvcp_amd.scene_io.save(scene, cornell)
    ppm = str(tmp_path / "out.ppm")
    r = subprocess.run([exe, scene, "40", "32", "3", "123.0", "1", ppm, "--cosine"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    from rvcp_amd import interactive
    want = _gpu(cornell, 40, 32, 123.0, spp=3)[0]
    assert np.array_equal(interactive.read_ppm(ppm), want[..., :3])
    r = subprocess.run([exe, scene, "40", "32", "3", "123.0", "1", ppm, "--cosin"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


# ----------------------------------------------------------------------------- the estimator
def closed_cornell():
    """The Cornell box with its open front closed by a white quad at z = -275 (two faces after
    the 32 existing ones), and a camera inside it: no ray can miss, so the shader's unattenuated
    miss term, which makes the modes' expectations differ on the open box, cannot act."""
    base = rvcp_amd.Scene.default()
    v, f = base.mesh.aligned_vertices(), base.mesh.aligned_faces()
    assert len(f) == 32
    nv = np.zeros(4, rvcp_amd.scene.VERTEX_DTYPE)
    nv["position"][:, :3] = np.float32([[-275, 0, -275], [275, 0, -275], [275, 548.8, -275], [-275, 548.8, -275]])
    nv["normal"][:, :3] = np.float32([0, 0, 1])
    nf = np.zeros(2, rvcp_amd.scene.FACE_DTYPE)
    nf["vertices"] = len(v) + np.uint32([[0, 1, 2], [0, 2, 3]])
    nf["material_id"] = 0
    mesh = rvcp_amd.scene.ArrayMesh(np.concatenate([v, nv]), np.concatenate([f, nf]))
    cam = rvcp_amd.Camera.new([0, 274.4, -255], [0, 274.4, 275], 0.1, 10000.0, 90.0, 150.0, 5.0)
    return rvcp_amd.Scene(cam, list(base.materials), [], mesh)


def _mean_frames(rt, sc, W, H, times):
    acc = np.zeros((H, W, 3), np.float64)
    for t in times:
        acc += rt.render_push(sc.push_constant(float(t)), W, H, want_linear=True)[1]
    return acc / len(times)


def _block_rms(a, b, k=8):
    def blocks(x):
        h, w = x.shape[:2]
        return x.reshape(h // k, k, w // k, k, 3).mean(axis=(1, 3))
    d = blocks(a) - blocks(b)
    return float(np.sqrt(np.mean(d * d)))


# Measured on an MI355X with the arithmetic of DESIGN.md §4.17: D(u1, u2) = 0.00185,
# D(c1, c2) = 0.00106, D(u1, c1) = 0.00252 (ratio 1.36), D(u2, c2) = 0.00219 (ratio 1.18).
def test_same_expectation_on_a_closed_box():
    """32 x 32, SPP = 64, attenuation stop off, float64 means over times 100..131 (set 1) and
    200..231 (set 2) in each mode; D = RMS difference of 8 x 8 block means.  The two modes must
    agree as well as two sets of uniform frames do, D(u1, c1) <= 2 D(u1, u2) -- 2 because the
    difference of two independent means of unequal noise is compared with that of two equal ones
    and one draw of it is itself noisy -- and the cosine sets must agree with each other no
    worse than the uniform ones, D(c1, c2) <= D(u1, u2).  The uniform frames are the oracle's,
    so D(u1, u2) = 0.00185 reproduces.  Tried in a scratch build: with the 1 / rr dropped from the
    weight (k = PI) D(u1, c1) is 0.0965, 52 times D(u1, u2), and this test fails (DESIGN.md
    §4.17).  On the open box the same measurement gives a ratio of 3.0 .. 3.2 (7.9 .. 8.2 with
    the attenuation stop at its default), for the reasons given there: documented, not asserted."""
    sc = closed_cornell()
    W = H = 32
    sets = {}
    with rvcp_amd.RayTracer(spp=64, attenuation_stop_eps=0.0) as rt:
        rt.upload_scene(sc)
        for mode, name in ((UNI, "u"), (COS, "c")):
            rt.sampling = mode
            sets[name + "1"] = _mean_frames(rt, sc, W, H, range(100, 132))
            sets[name + "2"] = _mean_frames(rt, sc, W, H, range(200, 232))
    d_uu = _block_rms(sets["u1"], sets["u2"])
    d_cc = _block_rms(sets["c1"], sets["c2"])
    d_uc = _block_rms(sets["u1"], sets["c1"])
    d_uc2 = _block_rms(sets["u2"], sets["c2"])
    print(f"closed box: D(u1,u2) {d_uu:.5f}, D(c1,c2) {d_cc:.5f}, D(u1,c1) {d_uc:.5f} "
          f"(ratio {d_uc / d_uu:.3f}), D(u2,c2) {d_uc2:.5f}; mean u {sets['u1'].mean():.5f}, "
          f"c {sets['c1'].mean():.5f}")
    assert d_uc <= 2.0 * d_uu, (d_uc, d_uu)
    assert d_cc <= d_uu, (d_cc, d_uu)


# cosine / uniform of this test's two errors, measured on an MI355X: 0.1140 / 0.1899 (the frames
# are deterministic, so the ratio reproduces); the gate is the midpoint of it and 1, as EDGE_GATE
# is set in test_svgf_cpu.  (Averaged over eight seeds the ratio is 0.72: profiles/
# sampling_time_1024sq.json.)
VARIANCE_RATIO = 0.600
VARIANCE_GATE = 0.5 * (VARIANCE_RATIO + 1.0)


def test_lower_variance(cornell):
    """Default Cornell box, 64 x 64, SPP = 4, one frame per mode (time 5.0), each against its
    own mode's mean of 32 frames x SPP 64 at other seeds (times 300..331): the L2 of the
    unclipped linear colours over all pixels."""
    W = H = 64
    err = {}
    for mode, name in ((UNI, "uniform"), (COS, "cosine")):
        with rvcp_amd.RayTracer(spp=64) as rt:
            rt.sampling = mode
            rt.upload_scene(cornell)
            mean = _mean_frames(rt, cornell, W, H, range(300, 332))
        with rvcp_amd.RayTracer(spp=4) as rt:
            rt.sampling = mode
            rt.upload_scene(cornell)
            frame = rt.render(W, H, 5.0, want_linear=True)[1].astype(np.float64)
        err[name] = float(np.sqrt(np.mean((frame - mean) ** 2)))
    ratio = err["cosine"] / err["uniform"]
    print(f"unclipped L2 at SPP 4: uniform {err['uniform']:.4f}, cosine {err['cosine']:.4f}, "
          f"ratio {ratio:.3f} (measured {VARIANCE_RATIO}), gate {VARIANCE_GATE}")
    assert ratio <= VARIANCE_GATE
