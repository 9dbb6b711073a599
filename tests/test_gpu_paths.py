"""Path queries on the GPU (rvcp_trace_paths_async and its family).

Every comparison is of float bits.  A frame's own rays and seeds are judged against the oracle's
linear frame and traversal count; rays that are no camera's against tests/paths_ref.py
(pyref.trace, pinned to the oracle by tests/test_paths_cpu.py); the tree contexts against a
context without the tree on the same rays."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import paths_ref
import rays_ref
import rvcp_amd
from conftest import scene_arrays
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)       # wave and block tails
SPP = 3                                             # of the rays that are no camera's


def dev(a):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def as_rays(rows):
    return np.ascontiguousarray(np.array(rows, f32)).view(abi.RAY_DTYPE).reshape(-1)


def trace(rt, rays, seeds, spp, stream=0):
    """(linear [n, 3] float32, traversals) of an asynchronous query on host arrays."""
    rays = np.ascontiguousarray(rays).view(abi.RAY_DTYPE).reshape(-1)
    seeds = np.ascontiguousarray(seeds, dtype=f32).reshape(-1)
    n = len(rays)
    assert len(seeds) == n
    d_r, d_s = dev(rays), dev(seeds)
    d_o = torch.full((n * 12,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), n, spp, d_o.data_ptr(), stream=stream)
    ms, trav = rt.paths_wait()
    assert ms >= 0.0
    return d_o.cpu().numpy().view(f32).reshape(n, 3), trav


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
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} rays differ, first ray {bad[0]}: got "
                           f"{g[bad[0]].view(f32)}, want {w[bad[0]].view(f32)}")


@pytest.fixture(scope="module")
def rotated(cornell):
    return rvcp_amd.scene.rotated_scene(cornell)


@pytest.fixture(scope="module")
def big(cornell):
    return rvcp_amd.scene.with_random_triangles(cornell, 2000)


# ------------------------------------------------------------------ 1. the frame identity
def frame_identity(sc, w, h, time, **kw):
    cfg = abi.make_config(**kw)
    push = sc.push_constant(time)
    want, _, want_trav = oracle.render(scene_arrays(sc), push, cfg, w, h)
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(sc)
        d_r, d_s = device_frame(rt, push, w, h)
        d_o = torch.full((w * h * 12,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), w * h, int(cfg["spp"]), d_o.data_ptr())
        _, trav = rt.paths_wait()
    got = d_o.cpu().numpy().view(f32)
    print(f"{w} x {h}, {kw}: traversals {trav} (oracle {want_trav})")
    same_bits(got, want, f"{w} x {h} frame {kw}")
    assert trav == want_trav


@pytest.mark.parametrize("spp", [1, 2, 5])
@pytest.mark.parametrize("which", ["cornell", "rotated"])
def test_frame_identity(cornell, rotated, which, spp):
    frame_identity(cornell if which == "cornell" else rotated, 24, 16, 7.0, spp=spp)


def test_frame_identity_over_many_waves(cornell):
    frame_identity(cornell, 96, 64, 1.0, spp=1)


def test_frame_identity_without_the_light_pick_quirk(cornell):
    frame_identity(cornell, 24, 16, 2.0, spp=2, lum_id_std140_quirk=0)


def test_frame_identity_short_paths_no_roulette(cornell):
    frame_identity(cornell, 24, 16, 3.0, spp=2, max_bounces=3, rr_probability=1.0)


def test_primary_seeds_equal_srand(cornell):
    w, h = 47, 39
    push = cornell.push_constant(2.5)
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        _, d_s = device_frame(rt, push, w, h)
    got = d_s.cpu().numpy().view(f32)
    want = paths_ref.frame_seeds(push["time"], w, h)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert ((got >= 0) & (got < 1)).all()


# ------------------------------------------------------------ 2. rays that are no camera's
@functools.lru_cache(maxsize=None)
def odd_pool():
    """96 rays over the Cornell box that no camera sends, their seeds, and the reference's
    radiance and traversals at SPP samples, computed once."""
    sc = rvcp_amd.Scene.default()
    arrays = scene_arrays(sc)
    rng = np.random.default_rng(0x9A7B5)
    lo, hi = np.array([-270.0, 5.0, -270.0]), np.array([270.0, 543.0, 270.0])
    rng_t = [0.01, 10000.0]

    def unit():
        d = rng.normal(size=3)
        return d / np.linalg.norm(d)

    sets = {}
    sets["inside"] = as_rays([np.concatenate([rng.uniform(lo, hi), unit(), rng_t]) for _ in range(24)])
    sets["half"] = as_rays([np.concatenate([rng.uniform(lo, hi), 0.5 * unit(), rng_t]) for _ in range(12)])
    sets["triple"] = as_rays([np.concatenate([rng.uniform(lo, hi), 3.0 * unit(), rng_t]) for _ in range(12)])
    # from outside the box: towards a point inside it, and the opposite way
    ins, outs = [], []
    for _ in range(12):
        o = np.array([rng.uniform(-600, 600), rng.uniform(700, 1200), rng.uniform(-600, 600)])
        if rng.random() < 0.5:
            o = np.array([rng.uniform(-200, 200), rng.uniform(100, 450), rng.uniform(-1500, -900)])
        d = rng.uniform(lo, hi) - o
        d = d / np.linalg.norm(d)
        ins.append(np.concatenate([o, d, rng_t]))
        outs.append(np.concatenate([o, -d, rng_t]))
    sets["outside_in"], sets["outside_away"] = as_rays(ins), as_rays(outs)
    # first hit the light: from just below it, towards points of its faces
    pos = arrays["vertices"]["position"][:, :3].astype(np.float64)
    lum = [int(i) for i in arrays["lum_face_ids"]]
    rows = []
    for k in range(12):
        tri = pos[arrays["faces"]["vertices"][lum[k % len(lum)]][:3]]
        b = rng.dirichlet([2.0, 2.0, 2.0])
        target = b @ tri
        o = target + np.array([rng.uniform(-40, 40), -rng.uniform(20, 120), rng.uniform(-40, 40)])
        d = target - o
        rows.append(np.concatenate([o, d / np.linalg.norm(d), rng_t]))
    sets["light"] = as_rays(rows)
    # first-segment ranges that end before, and begin behind, the first surface
    first = rays_ref.nearest(arrays, sets["inside"])
    hit = np.flatnonzero(first["face"] >= 0)[:12]              # (the box is open at the front)
    assert len(hit) == 12
    base, first = sets["inside"][hit].copy(), first[hit]
    base["t_max"][:6] = first["t"][:6] * f32(0.5)
    base["t_min"][6:] = first["t"][6:] * f32(1.001) + f32(0.01)
    sets["ranges"] = base
    rays = np.concatenate(list(sets.values()))
    assert len(rays) == 96
    assert (rays["t_max"] < 2.0 ** 24).all() and (np.abs(rays["d"]).max(axis=1) > 0).all()
    # the sets are what they are named for
    lum_set = set(lum)
    assert all(int(f) in lum_set for f in rays_ref.nearest(arrays, sets["light"])["face"])
    assert (rays_ref.nearest(arrays, sets["outside_away"])["face"] == -1).all()
    assert (rays_ref.nearest(arrays, sets["outside_in"])["face"] >= 0).all()
    r = rays_ref.nearest(arrays, sets["ranges"])
    assert (r["face"][:6] == -1).all() and (r["face"][6:] != first["face"][6:]).all()
    seeds = rng.random(len(rays), dtype=f32)
    assert ((seeds >= 0) & (seeds < 1)).all()
    lin, trav = paths_ref.trace_paths(sc, abi.make_config(spp=SPP), rays, seeds, SPP)
    lin.setflags(write=False)
    trav.setflags(write=False)
    # misses are 0.1 per sample; surfaces take more traversals than samples
    away = slice(60, 72)
    miss = paths_ref.F(0.0)
    for _ in range(SPP):
        miss = paths_ref.F(miss + paths_ref.F(paths_ref.F(0.1) / paths_ref.F(SPP)))
    assert (lin[away] == miss).all() and (trav[away] == SPP).all()
    assert (trav[:24] > SPP).any()
    return rays, seeds, lin, trav


def cycled(n):
    rays, seeds, lin, trav = odd_pool()
    idx = np.arange(n) % len(rays)
    return rays[idx], seeds[idx], lin[idx], int(trav[idx].sum())


def test_rays_that_are_no_cameras(cornell):
    rays, seeds, want, want_trav = odd_pool()
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        got, trav = trace(rt, rays, seeds, SPP)
    same_bits(got, want, "96 rays of no camera")
    assert trav == int(want_trav.sum())


# ---------------------------------------------------------------- 3. counts and independence
def test_every_ray_count(cornell):
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        for n in COUNTS:
            rays, seeds, want, want_trav = cycled(n)
            got, trav = trace(rt, rays, seeds, SPP)
            same_bits(got, want, f"n = {n}")
            assert trav == want_trav, n


def test_a_permutation_of_the_rays_permutes_the_results(cornell):
    rays, seeds, want, want_trav = cycled(1000)
    order = np.random.default_rng(11).permutation(1000)
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        got, trav = trace(rt, rays[order], seeds[order], SPP)
    same_bits(got, want[order], "permuted")
    assert trav == want_trav


# ------------------------------------------------------------------------ 4. tree contexts
def test_tree_contexts_equal_the_scan(big):
    w, h = 24, 16
    push = big.push_constant(4.0)
    odd, odd_seeds, _, _ = cycled(256)
    results = {}
    contexts = {"scan": dict(accel=abi.ACCEL_NONE), "hybrid": dict(accel=abi.ACCEL_BVH),
                "plain_tree": dict(accel=abi.ACCEL_BVH, specialize=abi.SPECIALIZE_OFF)}
    for name, kw in contexts.items():
        with rvcp_amd.RayTracer(spp=2, **kw) as rt:
            rt.upload_scene(big)
            d_r, d_s = device_frame(rt, push, w, h)
            rays = np.concatenate([d_r.cpu().numpy().view(abi.RAY_DTYPE), odd])
            seeds = np.concatenate([d_s.cpu().numpy().view(f32), odd_seeds])
            results[name] = (rays.tobytes(), seeds.tobytes()) + trace(rt, rays, seeds, 2)
    scan = results["scan"]
    assert (scan[2] != 0).any() and scan[3] > 2 * len(scan[2])
    for name in ("hybrid", "plain_tree"):
        r = results[name]
        assert r[0] == scan[0] and r[1] == scan[1], name           # the same rays and seeds
        same_bits(r[2], scan[2], name)
        assert r[3] == scan[3], name


# --------------------------------------------------------------------------- 5. bad rays
@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
def test_bad_rays_give_zeros_and_disturb_nothing(cornell, big, accel):
    sc = cornell if accel == abi.ACCEL_NONE else big
    n = 64 + 37                                                     # a full and a partial wave
    rays, seeds, _, _ = cycled(n)
    rays, seeds = rays.copy(), seeds.copy()
    bad_rays, bad_seeds = rays.copy(), seeds.copy()
    flat = bad_rays.view(f32).reshape(n, 8)
    rng = np.random.default_rng(5)
    where = rng.choice(n, size=27, replace=False)
    for j, i in enumerate(where[:24]):                              # each word, each bad value
        flat[i, j % 8] = (np.nan, np.inf, -np.inf)[j // 8]
    for i, s in zip(where[24:], (np.nan, -0.25, 1.0)):
        bad_seeds[i] = s
    bad = np.zeros(n, bool)
    bad[where] = True
    assert bad[:64].any() and bad[64:].any()
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(sc)
        clean, _ = trace(rt, rays, seeds, SPP)
        got, _ = trace(rt, bad_rays, bad_seeds, SPP)
        # a whole wave of nothing but rejected rays in front of good ones
        wave = np.concatenate([bad_rays[where[:1]].repeat(64), rays])
        wave_seeds = np.concatenate([bad_seeds[where[:1]].repeat(64), seeds])
        behind, _ = trace(rt, wave, wave_seeds, SPP)
    assert not got[bad].view(np.uint32).any()
    same_bits(got[~bad], clean[~bad], "the rays beside the bad ones")
    assert (clean[bad] != 0).any()
    assert not behind[:64].view(np.uint32).any()
    same_bits(behind[64:], clean, "behind a wave of rejected rays")


# -------------------------------------------------------------------------- 6. plumbing
def test_sync_equals_async(cornell):
    rays, seeds, want, want_trav = cycled(257)
    with rvcp_amd.RayTracer(spp=SPP) as rt:
        rt.upload_scene(cornell)
        a, trav = trace(rt, rays, seeds, SPP)
        s = rt.trace_paths(rays, seeds, SPP)
        assert rt.last_paths_ms is not None and rt.last_paths_ms >= 0.0
        assert rt.last_paths_traversals == trav == want_trav
        assert s.dtype == f32 and s.shape == (257, 3)
        same_bits(s, a, "sync against async")
        same_bits(rt.trace_paths(rays, seeds), a, "spp=None is the context's")
        same_bits(rt.trace_paths(rays[:1], seeds[:1], SPP), a[:1], "the staging reused")
    same_bits(a, want, "against the reference")


def test_sync_call_leaves_an_async_query_pending(cornell):
    L = abi.load()
    rays, seeds, want, want_trav = cycled(96)
    d_r, d_s = dev(rays), dev(seeds)
    d_o = torch.full((96 * 12,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), 96, SPP, d_o.data_ptr())
        s = rt.trace_paths(rays[:10], seeds[:10], SPP)
        same_bits(s, want[:10], "sync behind an async query")
        assert rt.last_paths_traversals == int(odd_pool()[3][:10].sum())
        ms, trav = rt.paths_wait()
        assert ms >= 0.0 and trav == want_trav                      # the async query's own count
        assert L.rvcp_paths_wait(rt.handle, None, None) == abi.RVCP_E_INVALID
        same_bits(d_o.cpu().numpy().view(f32), want, "the async query")
        rt.trace_paths(rays[:10], seeds[:10], SPP)                  # alone: nothing to wait for
        assert L.rvcp_paths_wait(rt.handle, None, None) == abi.RVCP_E_INVALID


def test_query_is_ordered_behind_a_pending_render(cornell):
    w = h = 96
    rays, seeds, want, _ = cycled(96)
    push = cornell.push_constant(5.0)
    d_r, d_s = dev(rays), dev(seeds)
    with rvcp_amd.RayTracer(spp=16) as rt:
        rt.upload_scene(cornell)
        frame_want = rt.render_push(push, w, h)
        d_rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        d_o = torch.zeros(96 * 12, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        rt.render_async(push, w, h, d_rgba.data_ptr())
        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), 96, SPP, d_o.data_ptr(),
                             stream=side.cuda_stream)
        rt.paths_wait()
        with torch.cuda.stream(side):
            frame = d_rgba.clone()
        side.synchronize()
        rt.wait()
    assert np.array_equal(frame.cpu().numpy().reshape(h, w, 4), frame_want)
    same_bits(d_o.cpu().numpy().view(f32), want, "behind a render")


def test_query_leaves_renders_statistics_and_ray_queries_alone(cornell):
    rays, seeds, want, _ = cycled(96)
    keys = ("traversals", "samples", "faces", "kernel_variant")
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        a = rt.render(48, 40, 11.0, want_linear=True)
        sa = rt.last_stats.copy()
        ha = rt.trace_rays(rays)
        got, _ = trace(rt, rays, seeds, SPP)
        b = rt.render(48, 40, 11.0, want_linear=True)
        sb = rt.last_stats.copy()
        hb = rt.trace_rays(rays)
    same_bits(got, want, "between renders")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for k in keys:
        assert sa[k] == sb[k], k
    assert ha.tobytes() == hb.tobytes()


def test_python_default_seeds_are_reproducible(cornell):
    rays, _, _, _ = odd_pool()
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        a = rt.trace_paths(rays, seed=3)
        b = rt.trace_paths(rays, seed=3)
        c = rt.trace_paths(rays, seed=4)
        want = rt.trace_paths(rays, np.random.default_rng(3).random(len(rays), dtype=f32), 2)
    same_bits(a, b, "the same seed")
    same_bits(a, want, "seeds of numpy.random.default_rng(seed)")
    assert a.tobytes() != c.tobytes()


def test_frame_identity_through_dynamic_queue_grabs(cornell):
    """More rays than a grid capped at one wave per SIMD holds lanes, so that waves come back to
    the queue's head: the frame's rays and seeds give the render's own linear frame (which the
    parity tests hold to the oracle's)."""
    w, h, spp = 384, 256, 1
    push = cornell.push_constant(9.0)
    with rvcp_amd.RayTracer(spp=spp, grid_waves_per_simd=1) as rt:
        rt.upload_scene(cornell)
        _, want = rt.render_push(push, w, h, want_linear=True)
        want_trav = int(rt.last_stats["traversals"])
        d_r, d_s = device_frame(rt, push, w, h)
        d_o = torch.full((w * h * 12,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rt.trace_paths_async(d_r.data_ptr(), d_s.data_ptr(), w * h, spp, d_o.data_ptr())
        _, trav = rt.paths_wait()
    same_bits(d_o.cpu().numpy().view(f32), want, "384 x 256 through the queue")
    assert trav == want_trav


# ------------------------------------------------------------------------------ 7. errors
def test_error_codes(cornell):
    L = abi.load()
    P = ctypes.c_void_p
    E = abi.RVCP_E_INVALID
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    buf = torch.full((8192,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = buf.data_ptr()
    r, s, o = d, d + 2048, d + 4096                                 # 4 rays, 4 seeds, 4 results
    h_rays, h_seeds = np.zeros(4, abi.RAY_DTYPE), np.zeros(4, f32)
    h_out = np.full((4, 3), 7.0, f32)

    def untouched():
        torch.cuda.synchronize()
        return bool((buf == 0xCD).all()) and bool((h_out == 7.0).all())

    with rvcp_amd.RayTracer(spp=1) as rt:
        h = rt.handle
        # before an upload
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, P(o), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 4, 1, abi.ptr(h_out), None, None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 4, 4, P(s), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_paths_wait(h, None, None) == E                # nothing enqueued
        rt.upload_scene(cornell)
        # NULL or zero arguments
        assert L.rvcp_trace_paths_async(h, None, P(s), 4, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), None, 4, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 0, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, None, None) == E
        assert L.rvcp_trace_paths(h, None, abi.ptr(h_seeds), 4, 1, abi.ptr(h_out), None, None) == E
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), None, 4, 1, abi.ptr(h_out), None, None) == E
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 0, 1, abi.ptr(h_out), None, None) == E
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 4, 1, None, None, None) == E
        assert L.rvcp_primary_seeds_async(h, None, 4, 4, P(s), None) == E
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 0, 4, P(s), None) == E
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 4, 0, P(s), None) == E
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 4, 4, None, None) == E
        # n_rays >= 2^31
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 1 << 31, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 0xFFFFFFFF, 1, P(o), None) == E
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 1 << 31, 1, abi.ptr(h_out), None, None) == E
        # spp outside 1..RVCP_SPP_MAP_MAX
        for spp in (0, abi.SPP_MAP_MAX + 1, 0xFFFFFFFF):
            assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, spp, P(o), None) == E
            assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 4, spp, abi.ptr(h_out), None, None) == E
        # alignment: 16 bytes for the rays, 4 for the seeds and the output
        assert L.rvcp_trace_paths_async(h, P(r + 8), P(s), 4, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s + 2), 4, 1, P(o), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, P(o + 2), None) == E
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 4, 4, P(s + 2), None) == E
        # an output that overlaps an input
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, P(r), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, P(r + 124), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(s), 4, 1, P(s + 12), None) == E
        assert L.rvcp_trace_paths_async(h, P(r), P(o + 44), 4, 1, P(o), None) == E
        # the primary rays' checks: W*H < 2^31, t_far x t_coef < 2^24
        assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 65536, 32768, P(s), None) == E
        far = push.copy()
        far["camera"]["t_far"] = 2.0 ** 24
        assert L.rvcp_primary_seeds_async(h, abi.ptr(far), 4, 4, P(s), None) == E
        # none of that wrote anything or left a query pending
        assert untouched()
        assert L.rvcp_paths_wait(h, None, None) == E
        # buffers that touch without overlapping are fine, at 4-byte addresses
        assert L.rvcp_trace_paths_async(h, P(r), P(r + 128 + 4), 4, 1, P(r + 128 + 20), None) == abi.RVCP_OK
        assert L.rvcp_paths_wait(h, None, None) == abi.RVCP_OK
        assert L.rvcp_paths_wait(h, None, None) == E


@pytest.mark.parametrize("kw", [dict(integrator=abi.INTEGRATOR_LEGACY), dict(n_gpus=2), dict(cosine=True)],
                         ids=["legacy", "two_gpus", "cosine"])
def test_unsupported_contexts(cornell, kw):
    L = abi.load()
    P = ctypes.c_void_p
    kw = dict(kw)
    cosine = kw.pop("cosine", False)
    buf = torch.full((8192,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = buf.data_ptr()
    h_rays, h_seeds = np.zeros(4, abi.RAY_DTYPE), np.zeros(4, f32)
    h_out = np.full((4, 3), 7.0, f32)
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    U = abi.RVCP_E_UNSUPPORTED
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(cornell)
        if cosine:
            rt.sampling = abi.SAMPLING_COSINE
        h = rt.handle
        assert L.rvcp_trace_paths_async(h, P(d), P(d + 2048), 4, 1, P(d + 4096), None) == U
        assert L.rvcp_trace_paths(h, abi.ptr(h_rays), abi.ptr(h_seeds), 4, 1, abi.ptr(h_out), None, None) == U
        if not cosine:                  # (the seeds do not depend on the bounce)
            assert L.rvcp_primary_seeds_async(h, abi.ptr(push), 4, 4, P(d), None) == U
        assert L.rvcp_paths_wait(h, None, None) == abi.RVCP_E_INVALID
        torch.cuda.synchronize()
        assert bool((buf == 0xCD).all()) and bool((h_out == 7.0).all())
        if cosine:                      # back to the uniform bounce, the query runs
            rt.sampling = abi.SAMPLING_UNIFORM
            assert L.rvcp_trace_paths_async(h, P(d), P(d + 2048), 4, 1, P(d + 4096), None) == abi.RVCP_OK
            assert L.rvcp_paths_wait(h, None, None) == abi.RVCP_OK
