"""Frames traced with a per-pixel sample count on the GPU (rvcp_render_spp_map_async, DESIGN.md
§4.18).

A pixel is one serial chain of samples on its own RNG stream, in the kernels and in the oracle
alike, so a pixel traced with count s must equal, bit for bit, the same pixel of the oracle's frame
at cfg.spp = s: a uniform map of s is rvcp_render_async at spp = s in every output and statistic,
and a seeded random map over the levels {1, 2, 3, 5, 8, 16} equals the oracle's frame of each
pixel's level with no pixel excluded -- through every map kernel (schedules 3, 4, 5, 6 and 10
generic, 3 and 6 specialised, the BVH path kernel, the hybrid; the schedule that ran is asserted),
on the scenes and at the frame sizes of test_gpu_importance.  Then the statistics, the clamp, the
cosine bounce (against the context's own frames of that mode: it has no oracle), the argument
checks (every rejected call is rejected on the host before any launch) and the default render
after a map render.  Tolerance throughout: linear RGB bits and RGBA8 bytes equal."""
import ctypes
import functools

import numpy as np
import pytest

import adaptive_ref as A
import oracle as O
import rvcp_amd
import tile_ties as T
from conftest import scene_arrays
from fuzz_scenes import _with_specks, fuzz_scene
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SPEC = abi.VARIANT_SPECIALIZED
OFF = abi.SPECIALIZE_OFF
UNI, COS = abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE
SIZES = [(9, 7), (48, 40), (416, 320)]   # one partly filled wave, tail forms, full waves
FUZZ_SEEDS = (2, 3, 5, 11)
HYBRID_SPECKS = 160
LEVELS = (1, 2, 3, 5, 8, 16)
HINT = 4
# (label, context arguments, schedule, specialised or None: either) -- every map kernel
GENERIC = [(f"schedule {v} generic", dict(kernel_variant=v, specialize=OFF), v, False)
           for v in (3, 4, 5, 6, 10)]
SPECIALISED = [(f"schedule {v} specialised", dict(kernel_variant=v), v, True) for v in (3, 6)]
BVH = [("BVH path kernel", dict(accel=abi.ACCEL_BVH, specialize=OFF), 7, False)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def random_map(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    return np.asarray(LEVELS, np.uint32)[rng.integers(0, len(LEVELS), (h, w))]


def map_frame(rt, push, w, h, m, hint=HINT):
    """One rvcp_render_spp_map_async frame of an open context: (rgba, linear, stats)."""
    d_map = dev(np.ascontiguousarray(m, dtype=np.uint32))
    d_rgba = torch.full((h * w * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    d_lin = torch.full((h * w * 12,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.render_spp_map_async(push, w, h, d_map.data_ptr(), hint, d_rgba.data_ptr(), d_lin.data_ptr())
    st = rt.wait().copy()
    torch.cuda.synchronize()
    return (d_rgba.cpu().numpy().reshape(h, w, 4),
            d_lin.cpu().numpy().view(np.float32).reshape(h, w, 3), st)


def map_render(sc, w, h, t, m, sampling=UNI, hint=HINT, **kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.sampling = sampling
        rt.upload_scene(sc)
        return map_frame(rt, sc.push_constant(t), w, h, m, hint)


def select(frames, m):
    """The frame whose pixel p is frames[m[p]]'s pixel p; frames: level -> [H, W, k]."""
    out = np.zeros_like(next(iter(frames.values())))
    for s, f in frames.items():
        out[m == s] = f[m == s]
    return out


def check(problems, label, got, want_rgba, want_lin, m, variant=None, spec=None):
    rgba, lin, st = got
    kv = int(st["kernel_variant"])
    if variant is not None and (kv & 15 != variant or (spec is not None and bool(kv & SPEC) != spec)):
        problems.append(f"{label}: kernel_variant {kv}, wanted schedule {variant}, specialised {spec}")
    diff = np.any(lin.view(np.uint32) != want_lin.view(np.uint32), axis=-1)
    if diff.any():
        at = np.argwhere(diff)[:3].tolist()
        problems.append(f"{label}: {int(diff.sum())} pixels differ in linear RGB, first at {at}, "
                        f"their counts {[int(m[y, x]) for y, x in at]}")
    if not np.array_equal(rgba, want_rgba):
        problems.append(f"{label}: {int(np.any(rgba != want_rgba, axis=-1).sum())} pixels differ in RGBA8")
    total = int(m.astype(np.uint64).sum())
    if int(st["samples"]) != total:
        problems.append(f"{label}: samples {int(st['samples'])}, wanted {total}")
    if int(st["traversals"]) - int(st["traversals_executed"]) != total - m.size:
        problems.append(f"{label}: traversals - executed {int(st['traversals']) - int(st['traversals_executed'])}, "
                        f"wanted {total - m.size}")


# ------------------------------------------------------------------- the oracle's frames, shared
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, config kwargs without spp, time, small: the specialised modules exist)."""
    if name == "cornell":
        return rvcp_amd.Scene.default(), {}, 123.0, True
    if name == "ties":
        mesh = T.tile_ties_mesh(T.SMALL)
        kw = T.path_config(mesh)
        return mesh.scene(), {k: v for k, v in kw.items() if k != "spp"}, 3.0, False
    kind, seed = name.split("-")
    sc, kw, _ = fuzz_scene(int(seed))
    if kind == "specks":
        sc = _with_specks(sc, HYBRID_SPECKS, int(seed))
    return sc, {k: v for k, v in kw.items() if k != "spp"}, 100.0 + int(seed), kind == "fuzz"


@functools.lru_cache(maxsize=None)
def oracle_levels(name, w, h):
    """level -> (linear, rgba) of the oracle's frames of scene `name`; read-only."""
    sc, kw, t, _ = _scene(name)
    out = {}
    for s in LEVELS:
        lin, rgba, _ = O.render(scene_arrays(sc), sc.push_constant(t), abi.make_config(spp=s, **kw), w, h)
        out[s] = (lin, rgba)
    return out


def expected(name, w, h, m):
    lv = oracle_levels(name, w, h)
    return select({s: f[1] for s, f in lv.items()}, m), select({s: f[0] for s, f in lv.items()}, m)


# ------------------------------------------------------------------------------ uniform maps
@pytest.mark.parametrize("kw", [dict(), dict(specialize=OFF), dict(kernel_variant=10),
                                dict(accel=abi.ACCEL_BVH, specialize=OFF)],
                         ids=["auto", "generic", "schedule10", "bvh"])
@pytest.mark.parametrize("s", [1, 2, 5])
def test_uniform_map_equals_the_uniform_render(cornell, s, kw):
    """A uniform map of s is rvcp_render_async at cfg.spp = s: linear bits, RGBA8, traversals,
    traversals_executed and samples -- whatever cfg.spp and the hint are."""
    W, H, t = 48, 40, 123.0
    with rvcp_amd.RayTracer(spp=s, **kw) as rt:
        rt.upload_scene(cornell)
        rgba, lin = rt.render(W, H, t, want_linear=True)
        want = rt.last_stats.copy()
    for hint in (s, 16):
        got = map_render(cornell, W, H, t, np.full((H, W), s, np.uint32), hint=hint, spp=7, **kw)
        assert np.array_equal(got[1].view(np.uint32), lin.view(np.uint32))
        assert np.array_equal(got[0], rgba)
        for k in ("traversals", "traversals_executed", "samples", "faces"):
            assert int(got[2][k]) == int(want[k]), (k, hint)
        if hint == s:
            assert int(got[2]["kernel_variant"]) == int(want["kernel_variant"])


# -------------------------------------------------------------------------------- mixed maps
SCENES = ["cornell"] + [f"fuzz-{s}" for s in FUZZ_SEEDS] + ["ties"]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_mixed_map_equals_the_oracle_per_pixel(name, w, h):
    sc, kw, t, small = _scene(name)
    m = random_map(w, h)
    assert set(np.unique(m).tolist()) == set(LEVELS) or w * h < 100
    want_rgba, want_lin = expected(name, w, h, m)
    problems = []
    for label, ckw, v, spec in GENERIC + (SPECIALISED if small else []) + BVH:
        check(problems, label, map_render(sc, w, h, t, m, spp=9, **ckw, **kw), want_rgba, want_lin,
              m, v, spec)
    assert not problems, problems


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_mixed_map_through_the_hybrid(seed, w, h):
    """The BVH hybrid: the leading big faces by the specialised scan (the map module's), the BVH
    over the rest."""
    name = f"specks-{seed}"
    sc, kw, t, _ = _scene(name)
    m = random_map(w, h, seed)
    want_rgba, want_lin = expected(name, w, h, m)
    problems = []
    got = map_render(sc, w, h, t, m, spp=9, accel=abi.ACCEL_BVH, **kw)
    check(problems, "BVH hybrid", got, want_rgba, want_lin, m, 7)
    assert not problems, problems
    assert int(got[2]["kernel_variant"]) & SPEC, "the hybrid's map module did not run"


def test_automatic_schedule_follows_the_hint(cornell):
    """The hint stands in for cfg.spp in the plan only: another schedule, the same bits."""
    w, h, t = 416, 320, 123.0
    m = random_map(w, h)
    want_rgba, want_lin = expected("cornell", w, h, m)
    problems, seen = [], set()
    for hint, kw in ((1, dict(specialize=OFF)), (256, dict(specialize=OFF)), (4, dict())):
        got = map_render(cornell, w, h, t, m, hint=hint, spp=20, **kw)
        check(problems, f"hint {hint}", got, want_rgba, want_lin, m)
        seen.add(int(got[2]["kernel_variant"]))
    assert not problems, problems
    assert {3, 6, 3 | SPEC} <= seen, seen      # 133 120 px x 256 >= kWideMinSamples: schedule 6


# -------------------------------------------------------------------------------- statistics
def test_two_row_bands_sum_the_oracles_traversals(cornell, cornell_arrays):
    W, H, t, top, a, b = 48, 40, 123.0, 17, 2, 5
    m = np.full((H, W), b, np.uint32)
    m[:top] = a
    push = cornell.push_constant(t)
    want = 0
    lin = np.zeros((H, W, 3), np.float32)
    for s, rect in ((a, (0, 0, W, top)), (b, (0, top, W, H - top))):
        o_lin, _, trav = O.render(cornell_arrays, push, abi.make_config(spp=s), W, H, rect=rect)
        lin[rect[1]:rect[1] + rect[3]] = o_lin
        want += trav
    for kw in (dict(), dict(kernel_variant=5)):
        rgba, got, st = map_render(cornell, W, H, t, m, **kw)
        assert np.array_equal(got.view(np.uint32), lin.view(np.uint32))
        assert int(st["traversals"]) == want
        assert int(st["samples"]) == W * (top * a + (H - top) * b)


def test_the_prepass_clamps_the_map(cornell, cornell_arrays):
    """0, 1, 256, 300 and 0xFFFFFFFF are traced as 1, 1, 256, 256, 256: the clamp is the pre-pass's
    (the map is device memory no host code validates)."""
    W, H, t = 9, 7, 123.0
    words = np.array([0, 1, 256, 300, 0xFFFFFFFF], np.uint32)
    m = words[np.random.default_rng(3).integers(0, len(words), (H, W))]
    m.ravel()[:5] = words
    c = A.clamp_map(m)
    assert set(np.unique(c).tolist()) == {1, 256}
    frames = {s: O.render(cornell_arrays, cornell.push_constant(t), abi.make_config(spp=s), W, H)
              for s in (1, 256)}
    want_lin = select({s: f[0] for s, f in frames.items()}, c)
    want_rgba = select({s: f[1] for s, f in frames.items()}, c)
    problems = []
    for label, ckw, v, spec in GENERIC[:1] + SPECIALISED[:1] + BVH:
        check(problems, label, map_render(cornell, W, H, t, m, **ckw), want_rgba, want_lin, c, v, spec)
    assert not problems, problems


# ---------------------------------------------------------------------------- cosine bounce
@pytest.mark.parametrize("w,h", SIZES[:2])
def test_cosine_bounce_per_pixel(cornell, w, h):
    """The same per-pixel equality in cosine mode, against the context's own rvcp_render_async
    frames of the cosine kernels at each level."""
    t = 123.0
    m = random_map(w, h)
    frames = {}
    for s in LEVELS:
        with rvcp_amd.RayTracer(spp=s, kernel_variant=1, specialize=OFF) as rt:
            rt.sampling = COS
            rt.upload_scene(cornell)
            rgba, lin = rt.render(w, h, t, want_linear=True)
            frames[s] = (lin, rgba)
    want_lin = select({s: f[0] for s, f in frames.items()}, m)
    want_rgba = select({s: f[1] for s, f in frames.items()}, m)
    uni = expected("cornell", w, h, m)[1]
    assert not np.array_equal(want_lin.view(np.uint32), uni.view(np.uint32))
    problems = []
    for label, ckw, v, spec in GENERIC + SPECIALISED + BVH:
        check(problems, label, map_render(cornell, w, h, t, m, sampling=COS, **ckw), want_rgba,
              want_lin, m, v, spec)
    assert not problems, problems


# ----------------------------------------------------------------------- arguments and state
P = lambda a: ctypes.c_void_p(a) if a else None           # noqa: E731


def test_rejected_calls_launch_nothing(cornell):
    W, H = 16, 8
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    d_map = dev(np.full((H, W), 2, np.uint32))
    d_out = torch.full((W * H * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    d_lin = torch.full((W * H * 12,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mp, op, lp = d_map.data_ptr(), d_out.data_ptr(), d_lin.data_ptr()

    def untouched(rt):
        assert rt._lib.rvcp_wait(rt.handle, None) == abi.RVCP_E_INVALID      # nothing in flight
        torch.cuda.synchronize()
        assert bool((d_out == 0xA5).all()) and bool((d_lin == 0xA5).all())

    def call(rt, push_=push, w=W, h=H, m=mp, hint=4, out=op):
        return rt._lib.rvcp_render_spp_map_async(rt.handle, abi.ptr(push_), w, h, P(m), hint, P(out),
                                                 P(lp), None)

    with rvcp_amd.RayTracer(spp=2) as rt:
        assert call(rt) == abi.RVCP_E_NO_SCENE
        untouched(rt)
        rt.upload_scene(cornell)
        for bad in (dict(push_=None), dict(w=0), dict(h=0), dict(m=0), dict(out=0), dict(hint=0),
                    dict(hint=257), dict(hint=0xFFFFFFFF), dict(w=1 << 16, h=1 << 15)):
            assert call(rt, **bad) == abi.RVCP_E_INVALID, bad
            untouched(rt)
        # a frame pending
        assert call(rt) == abi.RVCP_OK
        assert call(rt) == abi.RVCP_E_INVALID
        assert rt._lib.rvcp_set_adaptive(rt.handle, abi.ptr(abi.make_adaptive_params())) == abi.RVCP_E_INVALID
        rt.wait()
        torch.cuda.synchronize()
        assert not bool((d_out == 0xA5).all())
    d_out.fill_(0xA5)
    d_lin.fill_(0xA5)
    torch.cuda.synchronize()
    # schedules 1 and 2, mode 2 and n_gpus = 2
    for kw in (dict(kernel_variant=1), dict(kernel_variant=2), dict(kernel_variant=1, specialize=OFF)):
        with rvcp_amd.RayTracer(spp=2, **kw) as rt:
            rt.upload_scene(cornell)
            assert call(rt) == abi.RVCP_E_UNSUPPORTED, kw
            assert b"3-6" in rt._lib.rvcp_last_error(rt.handle)
            untouched(rt)
    with rvcp_amd.RayTracer(integrator=abi.INTEGRATOR_LEGACY) as rt:
        rt.upload_scene(cornell)
        assert call(rt) == abi.RVCP_E_UNSUPPORTED
        assert rt._lib.rvcp_set_adaptive(rt.handle, abi.ptr(abi.make_adaptive_params())) == abi.RVCP_E_UNSUPPORTED
        untouched(rt)
    with rvcp_amd.RayTracer(spp=2, n_gpus=2) as rt:
        rt.upload_scene(cornell)
        assert call(rt) == abi.RVCP_E_UNSUPPORTED
        assert rt._lib.rvcp_set_adaptive(rt.handle, abi.ptr(abi.make_adaptive_params())) == abi.RVCP_E_UNSUPPORTED
        untouched(rt)


def test_trivial_frame_is_black(cornell):
    W, H = 16, 8
    rgba, lin, st = map_render(cornell, W, H, 1.0, np.full((H, W), 3, np.uint32), max_bounces=0)
    assert not lin.any() and (rgba == np.uint8([0, 0, 0, 255])).all()
    assert int(st["traversals"]) == 0 and int(st["kernel_variant"]) == 0


@pytest.mark.parametrize("kw", [dict(), dict(specialize=OFF), dict(accel=abi.ACCEL_BVH)])
def test_default_render_after_a_map_render_is_the_oracles(cornell, cornell_arrays, kw):
    W, H, t = 48, 40, 123.0
    o_lin, o_rgba, o_trav = O.render(cornell_arrays, cornell.push_constant(t), abi.make_config(spp=3), W, H)
    m = random_map(W, H)
    want_rgba, want_lin = expected("cornell", W, H, m)
    with rvcp_amd.RayTracer(spp=3, **kw) as rt:
        rt.upload_scene(cornell)
        for _ in range(2):
            problems = []
            check(problems, "map", map_frame(rt, cornell.push_constant(t), W, H, m), want_rgba, want_lin, m)
            assert not problems, problems
            rgba, lin = rt.render(W, H, t, want_linear=True)
            assert np.array_equal(lin.view(np.uint32), o_lin.view(np.uint32))
            assert np.array_equal(rgba, o_rgba)
            assert int(rt.last_stats["traversals"]) == o_trav
            assert int(rt.last_stats["samples"]) == 3 * W * H


@pytest.mark.parametrize("name,ckw", [("cornell", dict()), ("specks-2", dict(accel=abi.ACCEL_BVH))],
                         ids=["specialised", "hybrid"])
def test_sampling_switches_between_default_and_map_renders(name, ckw):
    """One context keeps a module per render kind (default, map), each compiled for one bounce
    sampling: switching the sampling between renders of both kinds must hand every frame the module
    of its kind and mode.  Each frame of the sequence equals, in linear bits, RGBA8 bytes, traversal
    count and the kernel that ran, the same call on a fresh context in that mode -- which for the
    uniform bounce is the oracle's frame (of cfg.spp for a default render, of each pixel's level for
    a map render)."""
    W, H, SPP = 48, 40, 3
    sc, kw, t, _ = _scene(name)
    push, m = sc.push_constant(t), random_map(W, H)

    def frame(rt, is_map):
        if is_map:
            rgba, lin, st = map_frame(rt, push, W, H, m)
        else:
            rgba, lin = rt.render(W, H, t, want_linear=True)
            st = rt.last_stats
        return rgba, lin.view(np.uint32), int(st["traversals"]), int(st["kernel_variant"])

    def same(got, want):
        return all(np.array_equal(g, w) for g, w in zip(got, want))

    want = {}
    for mode in (UNI, COS):
        for is_map in (False, True):
            with rvcp_amd.RayTracer(spp=SPP, **ckw, **kw) as rt:
                rt.sampling = mode
                rt.upload_scene(sc)
                want[mode, is_map] = frame(rt, is_map)
            assert want[mode, is_map][3] & SPEC, "no specialised module ran"
    o_lin, o_rgba, o_trav = O.render(scene_arrays(sc), push, abi.make_config(spp=SPP, **kw), W, H)
    assert same(want[UNI, False][:3], (o_rgba, o_lin.view(np.uint32), o_trav))
    e_rgba, e_lin = expected(name, W, H, m)
    assert same(want[UNI, True][:2], (e_rgba, e_lin.view(np.uint32)))
    for is_map in (False, True):           # (the switch shows: the two modes' frames differ)
        assert not np.array_equal(want[UNI, is_map][1], want[COS, is_map][1])
    with rvcp_amd.RayTracer(spp=SPP, **ckw, **kw) as rt:
        rt.upload_scene(sc)
        steps = [(UNI, False), (UNI, True), (COS, True), (COS, False), (UNI, False), (UNI, True)]
        for i, (mode, is_map) in enumerate(steps):
            rt.sampling = mode
            assert same(frame(rt, is_map), want[mode, is_map]), (i, mode, is_map)
