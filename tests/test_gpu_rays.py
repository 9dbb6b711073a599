"""Ray queries on the GPU (rvcp_trace_rays_async and its family).

The reference is tests/rays_ref.py: the oracle's own triangle test walked over the faces in order
under the keep rule.  NEAREST results are compared with it bit for bit (face, t, b1, b2); ANY is
compared with NEAREST's face >= 0 on every ray this file traces (query() does both).  The tree
(accel = BVH) is judged against the scan by the classifier of tests/bvh_adversarial.py on that
module's own rays -- the rays the CPU model runs (tests/test_bvh_adversarial_cpu.py), here on
the device, with its v_rcp_f32 and its speculative leaf order."""
import ctypes
import functools

import numpy as np
import pytest

import bvh_adversarial as A
import oracle
import rays_ref
import rvcp_amd
from conftest import scene_arrays
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)       # wave and block tails
W, H = 47, 39
WELL_FORMED = ["ties", "degenerate"] + [f"offset2^{e}" for e in A.OFFSET_EXPONENTS]
FUZZ = [f"fuzz{s}" for s in range(8)]
MISS = np.zeros((), abi.RAY_HIT_DTYPE)
MISS["face"] = -1


def dev(a):
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def as_rays(rows):
    return np.ascontiguousarray(np.array(rows, f32)).view(abi.RAY_DTYPE).reshape(-1)


def trace(rt, rays, mode):
    rays = np.ascontiguousarray(rays).view(abi.RAY_DTYPE).reshape(-1)
    n = len(rays)
    d_r = dev(rays)
    d_o = torch.full((n * (4 if mode == abi.RAYS_ANY else 16),), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.trace_rays_async(d_r.data_ptr(), n, d_o.data_ptr(), mode)
    assert rt.rays_wait() >= 0.0
    return d_o.cpu().numpy().view(np.uint32 if mode == abi.RAYS_ANY else abi.RAY_HIT_DTYPE)


def query(rt, rays):
    """NEAREST of the rays; ANY is asserted to be 1 exactly where NEAREST reports a hit."""
    hits = trace(rt, rays, abi.RAYS_NEAREST)
    anyh = trace(rt, rays, abi.RAYS_ANY)
    bad = np.flatnonzero(anyh != (hits["face"] >= 0))
    assert len(bad) == 0, f"ANY differs from NEAREST on {len(bad)} rays, first {bad[:5]}: {anyh[bad[:5]]}"
    return hits


def same_hits(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} rays differ, first ray {bad[0]}: got "
                           f"{np.ascontiguousarray(got)[bad[0]]}, want {np.ascontiguousarray(want)[bad[0]]}")


def primary(push, w, h):
    return as_rays([oracle.sample_ray(push, w, h, x, y) for y in range(h) for x in range(w)])


def gbuffer(rt, push, w, h):
    buf = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.render_gbuffer_async(push, w, h, buf.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(abi.GBUFFER_DTYPE)


def device_primary(rt, push, w, h):
    buf = torch.full((w * h * 32,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.primary_rays_async(push, w, h, buf.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(abi.RAY_DTYPE)


@pytest.fixture(scope="module")
def rotated(cornell):
    return rvcp_amd.scene.rotated_scene(cornell)


@pytest.fixture(scope="module")
def big(cornell):
    return rvcp_amd.scene.with_random_triangles(cornell, 2000)


# ---------------------------------------------------------------------- 1. primary rays
@pytest.mark.parametrize("which", ["cornell", "rotated"])
def test_primary_rays_equal_sample_ray(cornell, rotated, which):
    sc = cornell if which == "cornell" else rotated
    push = sc.push_constant(2.0)
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(sc)
        got = device_primary(rt, push, 37, 23)
    want = primary(push, 37, 23)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------- 2. NEAREST against the reference
@functools.lru_cache(maxsize=None)
def cornell_pool():
    """{name: rays} over the Cornell box, and the reference's answers, computed once."""
    sc = rvcp_amd.Scene.default()
    arrays = scene_arrays(sc)
    rng = np.random.default_rng(0x4A75)
    sets = {"primary": primary(sc.push_constant(0.0), 37, 23)}
    lo, hi = np.array([-270.0, 5.0, -270.0]), np.array([270.0, 543.0, 270.0])
    rows = []
    for _ in range(512):                                    # incoherent, from inside the room
        d = rng.normal(size=3)
        rows.append(np.concatenate([rng.uniform(lo, hi), d / np.linalg.norm(d), [0.01, 10000.0]]))
    sets["incoherent"] = as_rays(rows)
    rows = []
    for _ in range(16):                                     # axis-parallel: two exact zeros
        o = rng.uniform(lo, hi)
        for k in range(3):
            for s in (-1.0, 1.0):
                d = np.zeros(3)
                d[k] = s
                rows.append(np.concatenate([o, d, [0.01, 10000.0]]))
    sets["axis"] = as_rays(rows)
    rows = []
    for _ in range(48):                                     # starting on the floor (y = 0 exactly)
        o = np.array([rng.uniform(-270, 270), 0.0, rng.uniform(-270, 270)])
        for d in (rng.normal(size=3), np.array([rng.normal(), 0.0, rng.normal()]), np.array([0.0, 1.0, 0.0])):
            d = d / np.linalg.norm(d)
            for tmin in (0.0, 0.01):                        # t_min = 0, and the configured one
                rows.append(np.concatenate([o, d, [tmin, 10000.0]]))
    sets["on_wall"] = as_rays(rows)
    # t_max exactly at, one ulp before and one ulp after a known hit
    base = np.concatenate([sets["primary"][::7], sets["incoherent"][::5]])
    ref = rays_ref.nearest(arrays, base)
    base, t = base[ref["face"] >= 0], ref["t"][ref["face"] >= 0]
    ends = []
    for tm in (t, np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf))):
        r = base.copy()
        r["t_max"] = tm
        ends.append(r)
    sets["t_max_ends"] = np.concatenate(ends)
    assert len(base) >= 100
    refs = {k: rays_ref.nearest(arrays, v) for k, v in sets.items()}
    # the ends do what they are for: the hit is kept at and after its t, lost one ulp before
    n = len(base)
    e = refs["t_max_ends"]
    assert (e["face"][:n] >= 0).all() and (e["face"][2 * n:] >= 0).all()
    assert np.array_equal(e["t"][:n].view(np.uint32), t.view(np.uint32))
    assert not np.array_equal(e[n:2 * n], e[:n])
    for k, v in refs.items():
        assert (v["face"] >= 0).sum() >= len(v) // 4, k
    return sets, refs


NONE_CONTEXTS = [dict(accel=abi.ACCEL_NONE), dict(accel=abi.ACCEL_NONE, specialize=abi.SPECIALIZE_OFF)]


@pytest.mark.parametrize("kw", NONE_CONTEXTS, ids=["default", "specialize_off"])
def test_nearest_equals_reference_on_every_ray_set(cornell, kw):
    sets, refs = cornell_pool()
    with rvcp_amd.RayTracer(spp=1, **kw) as rt:
        rt.upload_scene(cornell)
        for name, rays in sets.items():
            same_hits(query(rt, rays), refs[name], name)


@pytest.mark.parametrize("kw", NONE_CONTEXTS, ids=["default", "specialize_off"])
def test_nearest_at_every_ray_count(cornell, kw):
    """Wave and block tails: the first n rays of one seeded shuffle of all the sets."""
    sets, refs = cornell_pool()
    rays, ref = np.concatenate(list(sets.values())), np.concatenate(list(refs.values()))
    order = np.random.default_rng(7).permutation(len(rays))
    rays, ref = rays[order], ref[order]
    with rvcp_amd.RayTracer(spp=1, **kw) as rt:
        rt.upload_scene(cornell)
        for n in COUNTS:
            same_hits(query(rt, rays[:n]), ref[:n], f"n = {n}")


# ------------------------------------------------------------------ 3. against the G-buffer
def faces_of(g):
    return np.where(g["face"] == abi.GBUFFER_MISS, -1, g["face"].astype(np.int64)).astype(np.int32)


@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
@pytest.mark.parametrize("which", ["cornell", "big"])
def test_primary_query_equals_gbuffer(cornell, big, which, accel):
    sc = cornell if which == "cornell" else big
    push = sc.push_constant(1.0)
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(sc)
        g = gbuffer(rt, push, W, H)
        rays = device_primary(rt, push, W, H)
        hits = query(rt, rays)
    assert np.array_equal(hits["face"], faces_of(g))
    assert (hits["face"] >= 0).sum() >= W * H // 4
    # the hit point both ways: v0 + b1 e1 + b2 e2 is the texel's o + t d, to rounding
    v = sc.mesh.aligned_vertices()["position"][:, :3][sc.mesh.aligned_faces()["vertices"]].astype(np.float64)
    k = np.flatnonzero(hits["face"] >= 0)
    tri = v[hits["face"][k]]
    b1, b2 = hits["b1"][k].astype(np.float64)[:, None], hits["b2"][k].astype(np.float64)[:, None]
    p = tri[:, 0] * (1 - b1 - b2) + tri[:, 1] * b1 + tri[:, 2] * b2
    assert np.abs(p - g["position"][k]).max() < 0.05         # of a 550-unit room seen from 1300


def hybrid_scene(cornell):
    """As tests/test_gpu_bvh_adversarial.py: Cornell's 32 faces (the prefix), the ties mesh inside
    the room, and copies of the first twelve Cornell faces at the end, inside the tree."""
    mesh = A.ties_mesh()
    bv, bf = cornell.mesh.aligned_vertices(), cornell.mesh.aligned_faces()
    n = len(mesh.pos)
    nv = np.zeros(3 * n, bv.dtype)
    nv["position"][:, :3] = (mesh.pos.reshape(-1, 3) + f32([0, 274, 0])).astype(f32)
    nv["normal"][:, 1] = 1.0
    nf = np.zeros(n, bf.dtype)
    nf["vertices"] = len(bv) + np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    faces = np.concatenate([bf, nf, bf[:12].copy()])
    return rvcp_amd.Scene(cornell.camera, cornell.materials, [],
                          rvcp_amd.scene.ArrayMesh(np.concatenate([bv, nv]), faces)), len(faces)


def test_hybrid_ties_scene(cornell):
    sc, n = hybrid_scene(cornell)
    push = sc.push_constant(0.0)
    out = {}
    for accel in (abi.ACCEL_NONE, abi.ACCEL_BVH):
        with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
            rt.upload_scene(sc)
            g = gbuffer(rt, push, W, H)
            hits = query(rt, device_primary(rt, push, W, H))
        assert np.array_equal(hits["face"], faces_of(g))
        out[accel] = hits
    same_hits(out[abi.ACCEL_BVH], out[abi.ACCEL_NONE], "hybrid against the scan")
    f = out[abi.ACCEL_BVH]["face"]
    f = f[f >= 0]
    assert (f >= n - 12).sum() >= 100 and not (f < 12).any()    # the copies in the tree win


# ------------------------------------------------------- 4. the adversarial rays on the device
@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name.startswith("fuzz"):
        return A.fuzz_mesh(int(name[4:]))
    if name == "ties":
        return A.ties_mesh()
    if name == "degenerate":
        return A.degenerate_mesh()
    return A.offset_mesh(int(name.split("^")[1]))


def far_allowed(mesh):
    return 2.0 * 1000.0 * mesh.diag < A.T_CAP           # far_rays' own condition


@functools.lru_cache(maxsize=None)
def adversarial_report(name):
    """{set: (rays, scan hits, BVH hits or None)} of one mesh, every face in the tree
    (specialize = OFF: no hybrid prefix), plus make_rays' classes."""
    mesh = mesh_of(name)
    rays, tc, oc = A.make_rays(mesh)
    sets = {"make_rays": rays}
    if far_allowed(mesh):
        sets["far_rays"] = A.far_rays(mesh)
    sc = mesh.scene()
    out = {}
    with rvcp_amd.RayTracer(spp=1, accel=abi.ACCEL_NONE, specialize=abi.SPECIALIZE_OFF) as rt:
        rt.upload_scene(sc)
        for k, r in sets.items():
            out[k] = [r, query(rt, r), None]
    with rvcp_amd.RayTracer(spp=1, accel=abi.ACCEL_BVH, specialize=abi.SPECIALIZE_OFF) as rt:
        try:
            rt.upload_scene(sc)
        except abi.RvcpError as e:
            assert e.code == abi.RVCP_E_UNSUPPORTED, e
            return out, tc, oc
        for k, r in sets.items():
            out[k][2] = query(rt, r)
    return out, tc, oc


ADVERSARIAL = WELL_FORMED + FUZZ


@pytest.mark.parametrize("name", ADVERSARIAL)
def test_adversarial_scan_equals_reference(name):
    mesh = mesh_of(name)
    rep, _, _ = adversarial_report(name)
    assert "far_rays" in rep or not far_allowed(mesh)
    for k, (rays, scan, _) in rep.items():
        same_hits(scan, rays_ref.nearest(mesh.pos, rays), f"{name} {k}")


@pytest.mark.parametrize("name", ADVERSARIAL)
def test_adversarial_bvh_against_scan(name):
    mesh = mesh_of(name)
    rep, tc, oc = adversarial_report(name)
    pad_abs = A.builder_pad_abs(mesh.pos)
    for k, (rays, scan, bvh) in rep.items():
        if bvh is None:                 # RVCP_E_UNSUPPORTED, asserted in adversarial_report
            assert name not in WELL_FORMED
            print(f"{name}: upload unsupported, nothing compared")
            return
        r = rays.view(A.RAY_DTYPE)
        c, why = A.classify(mesh, r, scan, bvh, pad_abs)
        print(f"{name} {k}: {len(r)} rays, hits {int((scan['face'] >= 0).sum())}, differing "
              f"{int(np.count_nonzero(c))}, excused {int((c == 1).sum())}")
        assert not why, f"{name} {k}: {len(why)} unexcused rays, first {why[0]}"
        assert (c == 1).sum() <= A.EXCUSED_CAP * len(r), f"{name} {k}: {int((c == 1).sum())} excused"
        # where the two agree on face and t, b1 and b2 agree too: recomputed by the same operations
        same = c == 0
        assert scan[same].tobytes() == bvh[same].tobytes()


def test_adversarial_ties_near_origins():
    mesh = mesh_of("ties")
    rep, tc, oc = adversarial_report("ties")
    rays, scan, bvh = rep["make_rays"]
    assert bvh is not None
    near = np.isin(oc, [A.ORIGINS.index(k) for k in A.NEAR_ORIGINS])
    same_hits(bvh[near], scan[near], "ties, near origins")
    up = mesh.upper_duplicates()
    keys = [p.tobytes() for p in mesh.pos]
    copied = {keys[i] for i in np.flatnonzero(up)}
    has_copy = np.array([k in copied for k in keys]) & ~up
    f = bvh["face"][near]
    f = f[f >= 0]
    assert up[f].sum() >= A.MIN_TIES, f"only {int(up[f].sum())} near rays end on the later copy"
    assert not has_copy[f].any(), "a lower-indexed copy won a tie"


def test_adversarial_named_exits():
    unsupported = [n for n in ADVERSARIAL if adversarial_report(n)[0]["make_rays"][2] is None]
    print(f"not compared, unsupported: {unsupported or 'none'}")
    assert not set(unsupported) & set(WELL_FORMED)
    assert len(unsupported) < len(FUZZ) / 2


# -------------------------------------------------------------------------------- 5. ANY
@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
def test_any_in_a_split_wave(big, accel):
    """One wave whose first 32 rays hit at once -- face 0, the first the scan tests -- and whose
    last 32 miss: the loop may not be left while a lane still lacks its answer."""
    arrays = scene_arrays(big)
    tri = rays_ref.triangles(arrays)[0].reshape(3, 3).astype(np.float64)
    rng = np.random.default_rng(3)
    rows = []
    for _ in range(32):
        b = rng.dirichlet([2.0, 2.0, 2.0])
        q = b @ tri
        rows.append(np.concatenate([q - [0.0, 1e-3, 0.0], [0.0, 1.0, 0.0], [0.0, 10000.0]]))   # (the light faces down)
    for _ in range(32):                 # from in front of the room, away from it
        o = np.array([rng.uniform(-200, 200), rng.uniform(50, 500), -300.0])
        rows.append(np.concatenate([o, [0.0, 0.0, -1.0], [0.01, 10000.0]]))
    rays = as_rays(rows)
    ref = rays_ref.nearest(arrays, rays)
    assert (ref["face"][:32] == 0).all() and (ref["face"][32:] == -1).all()
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(big)
        same_hits(query(rt, rays), ref, "split wave")
        both = np.concatenate([rays[32:], rays[:32]])           # and the halves the other way round
        same_hits(query(rt, both), np.concatenate([ref[32:], ref[:32]]), "split wave, swapped")


# ---------------------------------------------------------------- 6. bad rays among good ones
@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
def test_non_finite_rays_miss_and_leave_their_wave_alone(cornell, big, accel):
    sc = cornell if accel == abi.ACCEL_NONE else big
    arrays = scene_arrays(sc)
    sets, _ = cornell_pool()
    good = np.concatenate([sets["primary"][100:132], sets["incoherent"][:32]])      # one wave
    waves, bad_at = [], []
    for word in range(8):
        for j, bad in enumerate((np.nan, np.inf, -np.inf)):
            w = good.copy()
            lane = (5 * word + 21 * j + 3) % 64
            w.view(f32).reshape(-1, 8)[lane, word] = bad
            waves.append(w)
            bad_at.append(len(bad_at) * 64 + lane)
    rays = np.concatenate(waves)
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(sc)
        clean = query(rt, good)
        got = query(rt, rays)
        assert (clean["face"] >= 0).sum() >= 32
        want = np.tile(clean, len(waves))
        want[bad_at] = MISS
        same_hits(got, want, "non-finite rays")
        # a zero direction and t_min > t_max go through the arithmetic: what the reference gives
        odd = good[:40].copy()
        odd["d"][:20] = 0.0
        odd["d"][5:10] = -0.0
        odd["t_min"][20:], odd["t_max"][20:] = good["t_max"][20:40], good["t_min"][20:40]
        ref = rays_ref.nearest(arrays, odd)
        same_hits(query(rt, odd), ref, "zero direction, t_min > t_max")
    same_hits(clean, rays_ref.nearest(arrays, good), "the clean wave")


# ------------------------------------------------------------------------------- 7. pick
@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
def test_pick_equals_gbuffer(cornell, accel):
    push = cornell.push_constant(0.0)
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(cornell)
        g = gbuffer(rt, push, W, H).reshape(H, W)
        hits = query(rt, device_primary(rt, push, W, H)).reshape(H, W)
        light = np.argwhere((g["face"] != abi.GBUFFER_MISS) & ((g["material"] & abi.GBUFFER_EMISSIVE) != 0))
        miss = np.argwhere(g["face"] == abi.GBUFFER_MISS)
        assert len(light) and len(miss)
        pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2),
                  (int(light[0][1]), int(light[0][0])), (int(miss[0][1]), int(miss[0][0]))]
        for x, y in pixels:
            hit = rt.pick(W, H, x, y)
            assert int(hit["face"]) == int(faces_of(g)[y, x]), (x, y)
            assert hit.tobytes() == hits[y, x].tobytes(), (x, y)
        assert int(rt.pick(W, H, *pixels[-1])["face"]) == -1 and int(rt.pick(W, H, *pixels[-2])["face"]) >= 0


# -------------------------------------------------------------------- 8. the sync wrapper
@pytest.mark.parametrize("accel", [abi.ACCEL_NONE, abi.ACCEL_BVH], ids=["none", "bvh"])
def test_sync_wrapper_equals_async(big, accel):
    sets, _ = cornell_pool()
    rays = np.concatenate([sets["primary"][::3], sets["incoherent"][:257]])
    with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
        rt.upload_scene(big)
        a = query(rt, rays)
        s = rt.trace_rays(rays)
        assert rt.last_rays_ms is not None and rt.last_rays_ms >= 0.0
        assert s.dtype == abi.RAY_HIT_DTYPE and s.tobytes() == a.tobytes()
        s_any = rt.trace_rays(rays, mode=abi.RAYS_ANY)
        assert s_any.dtype == np.uint32 and np.array_equal(s_any, a["face"] >= 0)
        assert rt.trace_rays(rays[:1]).tobytes() == a[:1].tobytes()         # (smaller: the staging is reused)


def test_sync_calls_leave_an_async_query_pending(cornell):
    """rvcp_trace_rays and rvcp_pick bracket their own query: an rvcp_trace_rays_async enqueued
    before them is still the one rvcp_rays_wait waits for, once, with its result intact."""
    L = abi.load()
    sets, refs = cornell_pool()
    rays = sets["incoherent"]
    d_r = dev(rays)
    d_o = torch.full((len(rays) * 16,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(cornell)
        rt.trace_rays_async(d_r.data_ptr(), len(rays), d_o.data_ptr())
        same_hits(rt.trace_rays(sets["axis"]), refs["axis"], "sync behind an async query")
        assert int(rt.pick(W, H, W // 2, H // 2)["face"]) >= 0
        assert rt.rays_wait() >= 0.0
        assert L.rvcp_rays_wait(rt.handle, None) == abi.RVCP_E_INVALID
        same_hits(d_o.cpu().numpy().view(abi.RAY_HIT_DTYPE), refs["incoherent"], "the async query")
        # and the synchronous calls alone leave nothing to wait for
        rt.trace_rays(sets["axis"])
        assert L.rvcp_rays_wait(rt.handle, None) == abi.RVCP_E_INVALID


# --------------------------------------------------------------- 9. ordering and isolation
def test_query_is_ordered_behind_a_pending_render(cornell):
    """A render pending on the context is not an error; a query on another stream is ordered
    after it: once the query is done, so is the frame."""
    w = h = 96
    sets, refs = cornell_pool()
    push = cornell.push_constant(5.0)
    d_r = dev(sets["incoherent"])
    n = len(sets["incoherent"])
    with rvcp_amd.RayTracer(spp=16) as rt:
        rt.upload_scene(cornell)
        want = rt.render_push(push, w, h)
        d_rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        d_o = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        rt.render_async(push, w, h, d_rgba.data_ptr())
        rt.trace_rays_async(d_r.data_ptr(), n, d_o.data_ptr(), abi.RAYS_NEAREST, stream=side.cuda_stream)
        rt.rays_wait()
        with torch.cuda.stream(side):
            frame = d_rgba.clone()
        side.synchronize()
        rt.wait()
    assert np.array_equal(frame.cpu().numpy().reshape(h, w, 4), want)
    same_hits(d_o.cpu().numpy().view(abi.RAY_HIT_DTYPE), refs["incoherent"], "behind a render")


def test_query_leaves_renders_and_statistics_alone(cornell):
    sets, refs = cornell_pool()
    keys = ("traversals", "samples", "faces", "kernel_variant")
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        a = rt.render(48, 40, 11.0, want_linear=True)
        sa = rt.last_stats.copy()
        same_hits(query(rt, sets["incoherent"]), refs["incoherent"], "between renders")
        rt.pick(48, 40, 3, 4)
        b = rt.render(48, 40, 11.0, want_linear=True)
        sb = rt.last_stats.copy()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for k in keys:
        assert sa[k] == sb[k], k


# ------------------------------------------------------------------------------ 10. errors
def test_error_codes(cornell):
    L = abi.load()
    P = ctypes.c_void_p
    E = abi.RVCP_E_INVALID
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = buf.data_ptr()
    host_rays = np.zeros(4, abi.RAY_DTYPE)
    host_out = np.zeros(4, abi.RAY_HIT_DTYPE)
    hit = np.zeros((), abi.RAY_HIT_DTYPE)
    with rvcp_amd.RayTracer(spp=1) as rt:
        h = rt.handle
        # before an upload
        assert L.rvcp_trace_rays_async(h, P(d), 4, 0, P(d + 1024), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 4, 0, abi.ptr(host_out), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 4, 4, P(d), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_pick(h, abi.ptr(push), 4, 4, 0, 0, abi.ptr(hit)) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_rays_wait(h, None) == E                   # nothing enqueued
        rt.upload_scene(cornell)
        # NULL or zero arguments
        assert L.rvcp_trace_rays_async(h, None, 4, 0, P(d + 1024), None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 0, 0, P(d + 1024), None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 4, 0, None, None) == E
        assert L.rvcp_trace_rays(h, None, 4, 0, abi.ptr(host_out), None) == E
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 0, 0, abi.ptr(host_out), None) == E
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 4, 0, None, None) == E
        assert L.rvcp_primary_rays_async(h, None, 4, 4, P(d), None) == E
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 0, 4, P(d), None) == E
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 4, 0, P(d), None) == E
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 4, 4, None, None) == E
        assert L.rvcp_pick(h, None, 4, 4, 0, 0, abi.ptr(hit)) == E
        assert L.rvcp_pick(h, abi.ptr(push), 4, 4, 0, 0, None) == E
        assert L.rvcp_pick(h, abi.ptr(push), 0, 4, 0, 0, abi.ptr(hit)) == E
        # n_rays >= 2^31 (as W*H for the G-buffer); rejected before anything is read
        assert L.rvcp_trace_rays_async(h, P(d), 1 << 31, 0, P(d + 1024), None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 0xFFFFFFFF, 1, P(d + 1024), None) == E
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 1 << 31, 0, abi.ptr(host_out), None) == E
        # a mode other than the two
        assert L.rvcp_trace_rays_async(h, P(d), 4, 2, P(d + 1024), None) == E
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 4, 7, abi.ptr(host_out), None) == E
        # alignment: 16 bytes, 4 for ANY's output
        assert L.rvcp_trace_rays_async(h, P(d + 8), 4, 0, P(d + 1024), None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 4, 0, P(d + 1024 + 8), None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 4, 1, P(d + 1024 + 2), None) == E
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 4, 4, P(d + 4), None) == E
        # x >= width, y >= height
        assert L.rvcp_pick(h, abi.ptr(push), 4, 4, 4, 0, abi.ptr(hit)) == E
        assert L.rvcp_pick(h, abi.ptr(push), 4, 4, 0, 4, abi.ptr(hit)) == E
        # the G-buffer's checks: W*H < 2^31, t_far x t_coef < 2^24
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 65536, 32768, P(d), None) == E
        far = push.copy()
        far["camera"]["t_far"] = 2.0 ** 24
        assert L.rvcp_primary_rays_async(h, abi.ptr(far), 4, 4, P(d), None) == E
        assert L.rvcp_pick(h, abi.ptr(far), 4, 4, 0, 0, abi.ptr(hit)) == E
        # none of that left a query pending; ANY's output may sit at a 4-byte address
        assert L.rvcp_rays_wait(h, None) == E
        assert L.rvcp_trace_rays_async(h, P(d), 4, 1, P(d + 1024 + 4), None) == abi.RVCP_OK
        assert L.rvcp_rays_wait(h, None) == abi.RVCP_OK
        assert L.rvcp_rays_wait(h, None) == E


@pytest.mark.parametrize("kw", [dict(integrator=abi.INTEGRATOR_LEGACY), dict(n_gpus=2)], ids=["legacy", "two_gpus"])
def test_unsupported_contexts(cornell, kw):
    L = abi.load()
    P = ctypes.c_void_p
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = buf.data_ptr()
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    hit = np.zeros((), abi.RAY_HIT_DTYPE)
    host_rays, host_out = np.zeros(4, abi.RAY_DTYPE), np.zeros(4, abi.RAY_HIT_DTYPE)
    U = abi.RVCP_E_UNSUPPORTED
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(cornell)
        h = rt.handle
        assert L.rvcp_trace_rays_async(h, P(d), 4, 0, P(d + 1024), None) == U
        assert L.rvcp_trace_rays(h, abi.ptr(host_rays), 4, 0, abi.ptr(host_out), None) == U
        assert L.rvcp_primary_rays_async(h, abi.ptr(push), 4, 4, P(d), None) == U
        assert L.rvcp_pick(h, abi.ptr(push), 4, 4, 0, 0, abi.ptr(hit)) == U
