"""Material scattering on the GPU (rvcp_set_materials, path_scatter_kernel).

Every comparison is of float bits.  With nothing specular in the scene the mode's kernel and
frame route are judged against the mode-off results (which the oracle tests pin); on the specular
scenes against tests/materials_ref.py through tests/golden/materials_frames.npz; the machine's
behaviour GPU against GPU; mode off on a specular scene against the C oracle."""
import os

import numpy as np
import pytest

import materials_ref as M
import oracle
import rvcp_amd
from conftest import scene_arrays
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
LAMB, SCAT = abi.MATERIALS_LAMBERTIAN, abi.MATERIALS_SCATTER
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "materials_frames.npz")
TIME = M.FIXTURE_TIME


def dev(a):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def query(rt, d_r, d_s, n, spp):
    """(linear [n, 3], traversals) of an asynchronous query on device tensors."""
    d_o = torch.full((n * 12,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), n, spp, d_o.data_ptr())
    ms, trav = rt.paths_wait()
    assert ms >= 0.0
    return d_o.cpu().numpy().view(f32).reshape(n, 3), trav


def trace(rt, rays, seeds, spp):
    rays = np.ascontiguousarray(rays).view(abi.RAY_DTYPE).reshape(-1)
    seeds = np.ascontiguousarray(seeds, dtype=f32).reshape(-1)
    return query(rt, dev(rays), dev(seeds), len(rays), spp)


def device_frame(rt, push, w, h):
    """The device's own primary rays and seeds of a frame, as device tensors."""
    d_r = torch.full((w * h * 32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_s = torch.full((w * h * 4,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.primary_rays_async(push, w, h, d_r.data_ptr())
    rt.primary_seeds_async(push, w, h, d_s.data_ptr())
    torch.cuda.synchronize()
    return d_r, d_s


def same_bits(got, want, what):
    g = np.ascontiguousarray(got, dtype=f32).reshape(-1, 3).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=f32).reshape(-1, 3).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} differ, first {bad[0]}: got "
                           f"{g[bad[0]].view(f32)}, want {w[bad[0]].view(f32)}")


@pytest.fixture(scope="module")
def specular():
    return rvcp_amd.scene.specular_cornell_scene()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def tree_scene():
    """specular_cornell_scene() with 2000 random triangles, every third of them metal and every
    third dielectric."""
    sc = rvcp_amd.scene.with_random_triangles(rvcp_amd.scene.specular_cornell_scene(), 2000)
    faces = sc.mesh.aligned_faces().copy()
    k = np.arange(2000)
    ids = faces["material_id"][32:]
    ids[k % 3 == 1] = 4         # the metal
    ids[k % 3 == 2] = 5         # the dielectric
    faces["material_id"][32:] = ids
    mesh = rvcp_amd.scene.ArrayMesh(sc.mesh.aligned_vertices(), faces)
    return rvcp_amd.scene.Scene(sc.camera, sc.materials, [], mesh)


# ------------------------------------------------ 1. identity: the mode on, nothing specular
@pytest.mark.parametrize("spp", [1, 2, 5])
@pytest.mark.parametrize("which", ["cornell", "rotated"])
def test_identity_without_specular_materials(cornell, which, spp):
    sc = cornell if which == "cornell" else rvcp_amd.scene.rotated_scene(cornell)
    w, h = 24, 16
    push = sc.push_constant(TIME)
    with rvcp_amd.RayTracer(spp=spp) as rt:
        rt.upload_scene(sc)
        d_r, d_s = device_frame(rt, push, w, h)
        off, off_trav = query(rt, d_r, d_s, w * h, spp)
        off_rgba, off_lin = rt.render(w, h, TIME, want_linear=True)
        off_stats = rt.last_stats.copy()
        assert int(off_stats["kernel_variant"]) != 11
        rt.materials = SCAT
        on, on_trav = query(rt, d_r, d_s, w * h, spp)
        on_rgba, on_lin = rt.render(w, h, TIME, want_linear=True)
        st = rt.last_stats
    same_bits(on, off, f"{which} spp {spp}: the query")
    assert on_trav == off_trav
    same_bits(off_lin, off, "the mode-off frame is its query")
    same_bits(on_lin, off_lin, f"{which} spp {spp}: the frame")
    assert np.array_equal(on_rgba, off_rgba)
    assert int(st["traversals"]) == int(off_stats["traversals"]) == on_trav
    assert int(st["samples"]) == w * h * spp and int(st["kernel_variant"]) == 11
    assert abi.KERNEL_NAMES[11] == "path_scatter_kernel"
    assert float(st["kernel_ms"]) >= float(st["main_kernel_ms"]) > 0.0


# ------------------------------------------------ 2. the new physics, against the restatement
@pytest.mark.parametrize("case", list(M.CASES))
def test_equals_the_restatement(golden, case):
    sc, kw, w, h = M.case_scene(case)
    spp = kw["spp"]
    push = sc.push_constant(TIME)
    want = golden[case + "/linear"]
    want_trav = int(golden[case + "/traversals"])
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.materials = SCAT
        rt.upload_scene(sc)
        d_r, d_s = device_frame(rt, push, w, h)
        got, trav = query(rt, d_r, d_s, w * h, spp)
        rgba, lin = rt.render(w, h, TIME, want_linear=True)
        st = rt.last_stats
        only_rgba = rt.render(w, h, TIME)            # without the caller's linear buffer
    print(f"{case}: traversals {trav} (restatement {want_trav})")
    same_bits(got, want, f"{case}: trace_paths")
    assert trav == want_trav
    same_bits(lin, want, f"{case}: render")
    assert np.array_equal(rgba, golden[case + "/rgba"]) and np.array_equal(only_rgba, rgba)
    assert int(st["traversals"]) == want_trav and int(st["samples"]) == w * h * spp
    assert int(st["traversals_executed"]) == want_trav - w * h * (spp - 1)


def test_mirror_is_the_restatements(golden, specular):
    rays, seeds = M.mirror_rays()
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        got = rt.trace_paths(rays, seeds, spp=1)
        trav = rt.last_paths_traversals
    same_bits(got, golden["mirror/linear"], "the mirror rays")
    assert trav == int(golden["mirror/traversals"].sum())


# ------------------------------------------------ 3. the machine, GPU against GPU
@pytest.fixture(scope="module")
def wide(specular):
    """96 x 64 rays and seeds of the specular scene and the default grid's result at SPP 1."""
    w, h = 96, 64
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        d_r, d_s = device_frame(rt, specular.push_constant(TIME), w, h)
        lin, trav = query(rt, d_r, d_s, w * h, 1)
    rays = d_r.cpu().numpy().view(abi.RAY_DTYPE)
    seeds = d_s.cpu().numpy().view(f32)
    lin.setflags(write=False)
    return rays, seeds, lin, trav


def test_dynamic_queue_grabs(specular):
    """384 x 256 = 98 304 rays through a grid capped at one wave per SIMD (at most 1024 waves =
    65 536 lanes on the MI355X's 1024 SIMDs): the static split hands out at most 64 rays a wave,
    so at least a third of the rays come from the queue's head, and every lane that takes one
    takes it after another ray -- its flags, kept first hit and specular bit are the previous
    ray's until the new ray sets them.  At SPP 2, so that the kept first hit is used.  Against
    the default grid (where a wave's static chunk is one ray per lane), as a query and through
    the frame route."""
    w, h = 384, 256
    push = specular.push_constant(TIME)
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        d_r, d_s = device_frame(rt, push, w, h)
        want, want_trav = query(rt, d_r, d_s, w * h, 2)
        frame = rt.render(w, h, TIME, want_linear=True)[1]
        assert int(rt.last_stats["traversals"]) == want_trav
    with rvcp_amd.RayTracer(spp=2, grid_waves_per_simd=1) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        got, trav = query(rt, d_r, d_s, w * h, 2)
        capped = rt.render(w, h, TIME, want_linear=True)[1]
        st = rt.last_stats
        iters = int(st["wave_iterations"])
    same_bits(frame, want, "the default grid's frame is its query")
    same_bits(got, want, "grid_waves_per_simd = 1: the query")
    same_bits(capped, want, "grid_waves_per_simd = 1: the frame")
    assert trav == want_trav == int(st["traversals"])
    assert iters > 0 and np.isfinite(want).all()
    # the frame holds what the flags are about: pixels whose first hit is metal, glass, neither
    assert len(np.unique(want.view(np.uint32), axis=0)) > w * h // 2


def test_permutation_counts_and_sync(specular, wide):
    rays, seeds, want, _ = wide
    perm = np.random.default_rng(11).permutation(len(rays))
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        base, _ = trace(rt, rays, seeds, 2)
        got, _ = trace(rt, rays[perm], seeds[perm], 2)
        same_bits(got, base[perm], "a permutation of the rays")
        # every count 1..130 against the first n of the 130-ray query (rays across the frame)
        pick = np.linspace(0, len(rays) - 1, 130).astype(int)
        r130, s130 = rays[pick], seeds[pick]
        full, _ = trace(rt, r130, s130, 2)
        same_bits(full, base[pick], "130 rays of the frame")
        d_r, d_s = dev(r130), dev(s130)
        for n in range(1, 131):
            part, _ = query(rt, d_r, d_s, n, 2)
            same_bits(part, full[:n], f"{n} rays")
        sync = rt.trace_paths(r130, s130, spp=2)
        same_bits(sync, full, "rvcp_trace_paths")
    assert not np.array_equal(base.view(np.uint32), want.view(np.uint32))     # SPP 2 is not SPP 1


# ------------------------------------------------ 4. the tree
def test_tree_equals_scan():
    sc = tree_scene()
    w, h, spp = 24, 16, 2
    push = sc.push_constant(TIME)
    res = {}
    for accel in (abi.ACCEL_NONE, abi.ACCEL_BVH):
        with rvcp_amd.RayTracer(spp=spp, accel=accel) as rt:
            rt.materials = SCAT
            rt.upload_scene(sc)
            d_r, d_s = device_frame(rt, push, w, h)
            q = query(rt, d_r, d_s, w * h, spp)
            rgba, lin = rt.render(w, h, TIME, want_linear=True)
            res[accel] = (q, rgba, lin, int(rt.last_stats["traversals"]))
            # bad rays and seeds give zeros and disturb no neighbour
            rays = d_r.cpu().numpy().view(abi.RAY_DTYPE).copy()
            seeds = d_s.cpu().numpy().view(f32).copy()
            bad = [3, 64, 65, 200]
            rays["d"][3, 1] = np.nan
            rays["o"][64, 0] = np.inf
            seeds[65] = 1.0
            seeds[200] = np.nan
            got, _ = trace(rt, rays, seeds, spp)
            assert not got[bad].view(np.uint32).any()
            keep = np.setdiff1d(np.arange(w * h), bad)
            same_bits(got[keep], q[0][keep], f"accel {accel}: neighbours of rejected rays")
    (qs, ts), (qb, tb) = res[abi.ACCEL_NONE][0], res[abi.ACCEL_BVH][0]
    same_bits(qb, qs, "the tree's query")
    assert tb == ts
    same_bits(res[abi.ACCEL_BVH][2], res[abi.ACCEL_NONE][2], "the tree's frame")
    same_bits(res[abi.ACCEL_NONE][2], qs, "the frame is its query")
    assert np.array_equal(res[abi.ACCEL_BVH][1], res[abi.ACCEL_NONE][1])
    assert res[abi.ACCEL_BVH][3] == res[abi.ACCEL_NONE][3] == ts


# ------------------------------------------------ 5. mode off on the specular scene
def test_mode_off_is_the_oracles_lambertian_frame(specular, golden):
    w, h, spp = 24, 16, 2
    push = specular.push_constant(TIME)
    o_lin, o_rgba, o_trav = oracle.render(scene_arrays(specular), push, abi.make_config(spp=spp), w, h)
    with rvcp_amd.RayTracer(spp=spp) as rt:
        rt.upload_scene(specular)
        assert rt.materials == LAMB
        d_r, d_s = device_frame(rt, push, w, h)
        for step in ("before", "after"):
            rgba, lin = rt.render(w, h, TIME, want_linear=True)
            same_bits(lin, o_lin, f"{step}: the frame")
            assert np.array_equal(rgba, o_rgba) and int(rt.last_stats["traversals"]) == o_trav
            q, trav = query(rt, d_r, d_s, w * h, spp)
            same_bits(q, o_lin, f"{step}: the query")
            assert trav == o_trav
            if step == "before":
                rt.materials = SCAT
                assert rt.materials == SCAT
                same_bits(rt.render(w, h, TIME, want_linear=True)[1], golden["default/linear"], "on")
                rt.materials = LAMB
                assert rt.materials == LAMB
    assert not np.array_equal(o_lin.view(np.uint32), golden["default/linear"].view(np.uint32))


# ------------------------------------------------ 6. contracts
def test_bad_rays_and_seeds_on_the_scan(specular, wide):
    rays, seeds, _, _ = wide
    rays, seeds = rays[:300].copy(), seeds[:300].copy()
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        want, _ = trace(rt, rays, seeds, 2)
        bad = [0, 63, 64, 299]
        rays["t_max"][0] = np.inf
        rays["d"][63, 2] = np.nan
        seeds[64] = -0.25
        seeds[299] = 1.5
        got, _ = trace(rt, rays, seeds, 2)
    assert not got[bad].view(np.uint32).any()
    keep = np.setdiff1d(np.arange(300), bad)
    same_bits(got[keep], want[keep], "neighbours of rejected rays")


def test_render_denoised_is_its_composition(specular):
    w, h = 32, 24
    push = specular.push_constant(TIME)
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.materials = SCAT
        rt.upload_scene(specular)
        rgba, lin = rt.render_denoised(w, h, TIME, want_linear=True)
        assert int(rt.last_stats["kernel_variant"]) == 11
        d_lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        d_raw = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        d_g = torch.zeros((h * w * 32,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        d_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rt.render_async(push, w, h, d_raw.data_ptr(), d_lin.data_ptr())
        rt.wait()
        rt.render_gbuffer_async(push, w, h, d_g.data_ptr())
        rt.denoise_async(d_lin.data_ptr(), d_g.data_ptr(), w, h, d_out.data_ptr(), d_rgba.data_ptr())
        rt.denoise_wait()
        torch.cuda.synchronize()
    same_bits(lin, d_out.cpu().numpy(), "render_denoised")
    assert np.array_equal(rgba, d_rgba.cpu().numpy().view(np.uint8).reshape(h, w, 4))


def test_refusals_leave_the_context_usable(specular, golden):
    U, w, h = abi.RVCP_E_UNSUPPORTED, 24, 16
    push = specular.push_constant(TIME)
    out = torch.zeros((2, h, w), dtype=torch.int32, device="cuda")
    spp_map = torch.ones((h, w), dtype=torch.int32, device="cuda")
    P = lambda t: t.data_ptr()      # noqa: E731
    with rvcp_amd.RayTracer(spp=2) as rt:
        L, ctx = rt._lib, rt.handle
        rt.upload_scene(specular)
        rt.materials = SCAT
        pushes = np.stack([np.ascontiguousarray(push, dtype=rvcp_amd.scene.PUSH_DTYPE)] * 2)
        assert L.rvcp_render_frames_async(ctx, abi.ptr(pushes), 2, w, h, 0, 1, abi.ptr(P(out)),
                                          None, None) == U
        assert "batch" in L.rvcp_last_error(ctx).decode()
        p1 = np.ascontiguousarray(push, dtype=rvcp_amd.scene.PUSH_DTYPE)
        assert L.rvcp_render_shard_async(ctx, abi.ptr(p1), w, h, 0, 2, abi.ptr(P(out)), None,
                                         None) == U
        assert L.rvcp_render_spp_map_async(ctx, abi.ptr(p1), w, h, abi.ptr(P(spp_map)), 2,
                                           abi.ptr(P(out)), None, None) == U
        assert L.rvcp_set_sampling(ctx, abi.SAMPLING_COSINE) == U
        assert rt.sampling == abi.SAMPLING_UNIFORM
        assert L.rvcp_sync_stats(ctx, None) == abi.RVCP_E_INVALID        # nothing was launched
        for bad in (2, -1, 77):
            assert L.rvcp_set_materials(ctx, bad) == abi.RVCP_E_INVALID
        assert L.rvcp_get_materials(ctx, None) == abi.RVCP_E_INVALID
        assert rt.materials == SCAT
        same_bits(rt.render(w, h, TIME, want_linear=True)[1], golden["default/linear"], "after")
        # the other direction: a cosine context refuses the mode
        rt.materials = LAMB
        rt.sampling = abi.SAMPLING_COSINE
        assert L.rvcp_set_materials(ctx, SCAT) == U and rt.materials == LAMB
    with rvcp_amd.RayTracer(integrator=abi.INTEGRATOR_LEGACY) as rt:
        assert rt._lib.rvcp_set_materials(rt.handle, SCAT) == U
        rt.materials = LAMB
    with rvcp_amd.RayTracer(spp=1, n_gpus=2) as rt:
        assert rt._lib.rvcp_set_materials(rt.handle, SCAT) == U and rt.materials == LAMB


def test_pending_frame_upload_and_validation(specular, golden):
    w, h = 24, 16
    out = torch.zeros((64, 64), dtype=torch.int32, device="cuda")
    with rvcp_amd.RayTracer(spp=2) as rt:
        L, ctx = rt._lib, rt.handle
        rt.upload_scene(specular)
        rt.render_async(specular.push_constant(1.0), 64, 64, out.data_ptr())
        assert L.rvcp_set_materials(ctx, SCAT) == abi.RVCP_E_INVALID         # as rvcp_set_sampling
        assert rt.materials == LAMB
        rt.wait()
        rt.materials = SCAT
        rt.upload_scene(specular)                                            # survives an upload
        assert rt.materials == SCAT
        same_bits(rt.render(w, h, TIME, want_linear=True)[1], golden["default/linear"], "re-upload")
        # an upload that breaks a rule is refused with the mode on, and names the material
        for field, value, word in (("fuzz", 1.5, "4"), ("fuzz", np.nan, "4"), ("fuzz", -0.1, "4"),
                                   ("refraction_ratio", 0.0, "5"), ("refraction_ratio", np.inf, "5")):
            mats = specular.aligned_materials().copy()
            mats[field][int(word)] = value
            with pytest.raises(abi.RvcpError) as e:
                rt.upload_arrays(mats, specular.mesh.aligned_vertices(),
                                 specular.mesh.aligned_faces(), specular.luminous_face_ids())
            assert e.value.code == abi.RVCP_E_INVALID and "material " + word in str(e.value)
        same_bits(rt.render(w, h, TIME, want_linear=True)[1], golden["default/linear"],
                  "the scene of before the refused uploads")
        # with the mode off nothing new is validated; setting the mode then is refused
        rt.materials = LAMB
        mats = specular.aligned_materials().copy()
        mats["fuzz"][4] = 1.5
        rt.upload_arrays(mats, specular.mesh.aligned_vertices(), specular.mesh.aligned_faces(),
                         specular.luminous_face_ids())
        rt.render(w, h, TIME)
        assert L.rvcp_set_materials(ctx, SCAT) == abi.RVCP_E_INVALID
        assert "material 4" in L.rvcp_last_error(ctx).decode() and rt.materials == LAMB


def test_a_change_drops_the_histories(specular):
    W = H = 32
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(specular)
        rt.materials = SCAT
        raw = rt.render(W, H, 1.0, want_linear=True)[1]
        t1 = rt.render_temporal(W, H, 1.0, want_linear=True, want_history=True)
        t2 = rt.render_temporal(W, H, 2.0, want_linear=True, want_history=True)
        s1 = rt.render_svgf(W, H, 1.0, want_linear=True, want_history=True)
        s2 = rt.render_svgf(W, H, 2.0, want_linear=True, want_history=True)
        for a, b in ((t1, t2), (s1, s2)):
            assert np.isfinite(b[1]).all()
            assert int(b[2].max()) == int(a[2].max()) + 1               # the history grew
        same_bits(t1[1], raw, "the first accumulated frame is the mode's frame")
        rt.materials = SCAT                                             # no change: they stay
        assert int(rt.render_temporal(W, H, 3.0, want_history=True)[1].max()) == int(t2[2].max()) + 1
        rt.materials = LAMB                                             # a change: both restart
        t4 = rt.render_temporal(W, H, 4.0, want_history=True)
        s4 = rt.render_svgf(W, H, 4.0, want_history=True)
        assert int(t4[1].max()) == int(t1[2].max()) and int(s4[1].max()) == int(s1[2].max())


@pytest.mark.parametrize("chain", ["taa", "upsample"])
def test_a_change_drops_the_taa_and_upsampling_states(specular, chain):
    """After a change of the mode (here there and back, so that the frames are comparable) the
    TAA resolve's and the upsampling's states are gone and their jitter sequences restart: the
    next frame of each chain is bit for bit the first frame of a fresh context's sequence."""
    W = H = 32
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(specular)
        rt.materials = SCAT
        if chain == "taa":
            rt.taa = True
        else:
            rt.taa_upsample = 2
        for render in (rt.render_temporal, rt.render_svgf):
            first = render(W, H, 1.0, want_linear=True)[1]
            second = render(W, H, 1.0, want_linear=True)[1]
            assert not np.array_equal(first.view(np.uint32), second.view(np.uint32))
            rt.materials = SCAT                                         # no change: the state stays
            third = render(W, H, 1.0, want_linear=True)[1]
            assert not np.array_equal(third.view(np.uint32), first.view(np.uint32))
            rt.materials = LAMB
            rt.materials = SCAT
            same_bits(render(W, H, 1.0, want_linear=True)[1], first, f"{chain}: restarted")


def test_headless_loop_and_c_example(tmp_path, specular):
    import subprocess
    from rvcp_amd import interactive
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(specular)
        interactive.run_headless(rt, specular, 1, 32, 24, fixed_dt=0.0, time_seed=lambda i: 1.0,
                                 on_fps=lambda n: None, materials=SCAT)
        assert rt.materials == SCAT
        want = rt.render(40, 32, 123.0)
        interactive.run_headless(rt, specular, 1, 32, 24, fixed_dt=0.0, time_seed=lambda i: 1.0,
                                 on_fps=lambda n: None)                 # None: the mode stays
        assert rt.materials == SCAT
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "build", "rvcp_render")
    scene = str(tmp_path / "s.rvcpscn")
    rvcp_amd.scene_io.save(scene, specular)
    ppm = str(tmp_path / "out.ppm")
    r = subprocess.run([exe, scene, "40", "32", "2", "123.0", "1", ppm, "--materials"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(interactive.read_ppm(ppm), want[..., :3])
