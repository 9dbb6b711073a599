"""Albedo demodulation on the GPU: rvcp_demodulate_async and
rvcp_remodulate_async bit-identical to the numpy restatement (tests/albedo_ref.py) with no pixel
excluded, the fused store equal to oracle.gamma_u8 of the remodulated floats under both
unorm_rules, in place equal to out of place, the optional outputs, the argument checks (every
rejected call is rejected on the host before any launch), the three chains with the switch set
against the library's own stateless composition and against the restatement, the switch's effect
on the histories, and a white scene on which the switch changes no byte."""
import ctypes

import numpy as np
import pytest

import albedo_ref as A
import denoise_ref as R
import svgf_ref as S
import temporal_ref as T
import rvcp_amd
from rvcp_amd import abi
from rvcp_amd import scene as _scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = np.float32
Material, MaterialType, vec3 = _scene.Material, _scene.MaterialType, _scene.vec3
checker_floor_scene, cornell_box = _scene.checker_floor_scene, _scene.cornell_box


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    """A numpy array's bytes in a torch device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def blank(nbytes, fill=0xA5):
    """An output buffer that starts from a pattern no result has."""
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def assert_same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ"


def floats(t, *shape):
    return t.cpu().numpy().view(np.float32).reshape(*shape)


# ---------------------------------------------------------------------------- scenes
def zero_channel_scene():
    """The Cornell box with a zero channel in two of its albedos (one of them twice)."""
    sc = cornell_box()
    sc.materials[0] = Material.new_lambertian(vec3(0.725, 0.0, 0.68))
    sc.materials[1] = Material.new_lambertian(vec3(0.0, 0.0, 0.05))
    return sc


def single_material_scene():
    """The Cornell box's mesh under one Lambertian material (and no light)."""
    sc = cornell_box()
    sc.materials = [Material.new_lambertian(vec3(0.5, 0.3, 0.9))]
    for f in sc.mesh.faces:
        f.material_id = 0
    return sc


def white_scene():
    """The Cornell box with every Lambertian albedo (1, 1, 1)."""
    sc = cornell_box()
    sc.materials = [m if m.ty == MaterialType.Light else Material.new_lambertian(vec3(1.0, 1.0, 1.0))
                    for m in sc.materials]
    return sc


SCENES = dict(cornell=cornell_box, zero=zero_channel_scene, single=single_material_scene)


@pytest.fixture(scope="module")
def tracers():
    """Per scene: its albedo table and one context per unorm_rule with the scene uploaded."""
    out = {}
    for name, make in SCENES.items():
        sc = make()
        rts = []
        for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST):
            rt = rvcp_amd.RayTracer(unorm_rule=rule)
            rt.upload_scene(sc)
            rts.append(rt)
        out[name] = (A.albedo_table(sc.aligned_materials()), rts)
    yield out
    for _, rts in out.values():
        for rt in rts:
            rt.close()


# ---------------------------------------------------------------------------- stateless steps
def gpu_demodulate(rt, c, g, in_place=False):
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_out = d_c if in_place else blank(W * H * 12)
    torch.cuda.synchronize()
    rt.demodulate_async(d_c.data_ptr(), d_g.data_ptr(), W, H, d_out.data_ptr())
    d_ms, r_ms = rt.albedo_wait()
    assert d_ms >= 0.0 and r_ms == 0.0
    if not in_place:                                     # the input is left as it was
        assert np.array_equal(d_c.cpu().numpy(), np.ascontiguousarray(c).view(np.uint8).reshape(-1))
    return floats(d_out, H, W, 3)


def gpu_remodulate(rt, e, g, want_lin=True, want_rgba=True):
    H, W = e.shape[:2]
    d_e, d_g = dev(e), dev(g)
    d_lin, d_rgba = blank(W * H * 12), blank(W * H * 4, 0)
    torch.cuda.synchronize()
    rt.remodulate_async(d_e.data_ptr(), d_g.data_ptr(), W, H, d_lin.data_ptr() if want_lin else 0,
                        d_rgba.data_ptr() if want_rgba else 0)
    d_ms, r_ms = rt.albedo_wait()
    assert d_ms == 0.0 and r_ms >= 0.0
    return floats(d_lin, H, W, 3), d_rgba.cpu().numpy().reshape(H, W, 4)


# ---------------------------------------------------------------------------- 1. kernel parity
# 1 x 1; one full block; a ragged last wave and a ragged last row of blocks; several blocks
SIZES = [(1, 1), (64, 4), (67, 5), (130, 9)]


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("W,H", SIZES)
def test_steps_match_numpy_restatement(tracers, W, H, scene):
    table, rts = tracers[scene]
    c, g = A.synthetic_case(W, H, seed=W * 1000 + H, n_materials=len(table))
    if W * H == 1:
        g["face"], g["material"] = 7, 0
    else:
        on = A._on_albedo(g, table)[0]
        flat = g.reshape(-1)
        assert on.any() and not on.all()
        assert (flat["face"] == A.MISS).any() and (flat["material"] & A.EMISSIVE).any()
        assert (flat["material"] == len(table)).any() and (flat["material"] == 0x7FFFFFFF).any()
        assert not c.reshape(-1, 3)[1].any() and c.max() == f32(1.0e4)
    want_e = A.demodulate(c, g, table)
    want_o = A.remodulate(want_e, g, table)
    for rule, rt in enumerate(rts):
        e = gpu_demodulate(rt, c, g)
        assert_same(e, want_e, f"irradiance (rule {rule})")
        assert_same(gpu_demodulate(rt, c, g, in_place=True), want_e, f"in place (rule {rule})")
        lin, rgba = gpu_remodulate(rt, e, g)
        assert_same(lin, want_o, f"colour (rule {rule})")
        assert np.array_equal(rgba, R.gamma_rgba(want_o, rule)), rule
        # either output alone agrees with both together, and the other buffer is untouched
        lin1, rgba1 = gpu_remodulate(rt, e, g, want_rgba=False)
        assert_same(lin1, lin, "only linear")
        assert not rgba1.any()
        lin2, rgba2 = gpu_remodulate(rt, e, g, want_lin=False)
        assert np.array_equal(rgba2, rgba)
        assert (lin2.view(np.uint8) == 0xA5).all()


def test_zero_channels_and_pass_through(tracers):
    """What the zero-channel scene is for: a zero albedo channel gives 0 in and 0 out; off pixels
    keep their bits through both steps."""
    table, rts = tracers["zero"]
    W, H = 67, 5
    c, g = A.synthetic_case(W, H, seed=3, n_materials=len(table))
    on = A._on_albedo(g, table)[0]
    e = gpu_demodulate(rts[0], c, g)
    o, _ = gpu_remodulate(rts[0], e, g)
    m = g["material"] & np.uint32(0x7FFFFFFF)
    for mat, ch in ((0, 1), (1, 0), (1, 1)):
        sel = on & (m == mat)
        assert sel.any() and not e[sel][:, ch].any() and not o[sel][:, ch].any()
    assert np.array_equal(bits(e)[~on], bits(c)[~on]) and np.array_equal(bits(o)[~on], bits(c)[~on])


# ---------------------------------------------------------------------------- 2. rejections
P = lambda a: ctypes.c_void_p(a) if a else None           # noqa: E731


@pytest.fixture(scope="module")
def api(cornell):
    """Device buffers of a 16 x 16 case and the two entry points as keyword calls on a context
    with the Cornell box uploaded; every output starts zeroed, and stays so through every
    rejected call."""
    L = abi.load()
    W = H = 16
    npx = W * H
    c, g = A.synthetic_case(W, H, seed=5, n_materials=4)
    tens = dict(lin=dev(c), gbuf=dev(g))
    outs = dict(out=torch.zeros(npx * 12 + 64, dtype=torch.uint8, device="cuda"),
                rgba=torch.zeros(npx * 4 + 64, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    rt = rvcp_amd.RayTracer(spp=2)
    rt.upload_scene(cornell)
    base = dict({k: t.data_ptr() for k, t in {**tens, **outs}.items()}, w=W, h=H, ctx=rt.handle)

    def demodulate(**kw):
        a = dict(base, **kw)
        return L.rvcp_demodulate_async(a["ctx"], P(a["lin"]), P(a["gbuf"]), a["w"], a["h"],
                                       P(a["out"]), None)

    def remodulate(**kw):
        a = dict(base, **kw)
        return L.rvcp_remodulate_async(a["ctx"], P(a["lin"]), P(a["gbuf"]), a["w"], a["h"],
                                       P(a["out"]), P(a["rgba"]), None)

    yield dict(L=L, rt=rt, h=rt.handle, base=base, npx=npx, demodulate=demodulate,
               remodulate=remodulate, inputs=(c, g), tens=tens)
    # nothing was launched by a rejected call: every output is still zero, every input intact
    torch.cuda.synchronize()
    clean = all(not t.cpu().numpy().any() for t in outs.values())
    intact = np.array_equal(tens["lin"].cpu().numpy(), np.ascontiguousarray(c).view(np.uint8).reshape(-1))
    rt.close()
    assert clean and intact


def test_api_rejects_null_zero_and_oversized_arguments(api):
    E = abi.RVCP_E_INVALID
    for name in ("lin", "gbuf", "out", "w", "h"):
        assert api["demodulate"](**{name: 0}) == E, name
    for name in ("lin", "gbuf", "w", "h"):
        assert api["remodulate"](**{name: 0}) == E, name
    assert api["remodulate"](out=0, rgba=0) == E                          # not both
    for call in (api["demodulate"], api["remodulate"]):
        assert call(ctx=None) == E
        assert call(w=65536, h=32768) == E                                # W * H = 2^31
        assert b"2^31" in api["L"].rvcp_last_error(api["h"])
    assert api["L"].rvcp_albedo_wait(api["h"], None, None) == E           # nothing was enqueued
    assert b"in flight" in api["L"].rvcp_last_error(api["h"])
    assert api["L"].rvcp_albedo_wait(None, None, None) == E
    assert api["L"].rvcp_set_demodulation(None, 1) == E
    assert api["L"].rvcp_get_demodulation(None, None) == E
    assert api["L"].rvcp_get_demodulation(api["h"], None) == E


def test_api_rejects_overlapping_buffers(api):
    E, b, npx = abi.RVCP_E_INVALID, api["base"], api["npx"]
    for kw in (dict(out=b["lin"] + 12), dict(out=b["lin"] + 12 * npx - 4), dict(out=b["gbuf"]),
               dict(out=b["gbuf"] + 32 * npx - 4), dict(lin=b["out"] + 12)):
        assert api["demodulate"](**kw) == E, kw
        assert b"overlap" in api["L"].rvcp_last_error(api["h"])
    for kw in (dict(out=b["lin"]), dict(out=b["lin"] + 12 * npx - 4), dict(out=b["gbuf"]),
               dict(rgba=b["lin"]), dict(rgba=b["gbuf"] + 32 * npx - 4), dict(rgba=b["out"]),
               dict(rgba=b["out"] + 12 * npx - 4), dict(out=0, rgba=b["lin"] + 8)):
        assert api["remodulate"](**kw) == E, kw
        assert b"overlap" in api["L"].rvcp_last_error(api["h"])


def test_api_needs_a_scene():
    L = abi.load()
    with rvcp_amd.RayTracer(spp=2) as rt:
        d = torch.zeros(16 * 16 * 32, dtype=torch.uint8, device="cuda")
        out = torch.zeros(16 * 16 * 12, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p, q = P(d.data_ptr()), P(out.data_ptr())
        assert L.rvcp_demodulate_async(rt.handle, p, p, 16, 16, q, None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_remodulate_async(rt.handle, p, p, 16, 16, q, None, None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_albedo_wait(rt.handle, None, None) == abi.RVCP_E_INVALID
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()


@pytest.mark.parametrize("kw", [dict(integrator=abi.INTEGRATOR_LEGACY), dict(n_gpus=2)])
def test_unsupported_contexts(cornell, kw):
    L = abi.load()
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(cornell)
        d = torch.zeros(16 * 16 * 32, dtype=torch.uint8, device="cuda")
        out = torch.zeros(16 * 16 * 12, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p, q = P(d.data_ptr()), P(out.data_ptr())
        assert L.rvcp_demodulate_async(rt.handle, p, p, 16, 16, q, None) == abi.RVCP_E_UNSUPPORTED
        assert L.rvcp_remodulate_async(rt.handle, p, p, 16, 16, q, None, None) == abi.RVCP_E_UNSUPPORTED


def test_switch_is_refused_while_a_frame_is_pending(api, cornell):
    rt, L = api["rt"], api["L"]
    W = H = 16
    d_rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert rt.demodulation is False
    rt.render_async(cornell.push_constant(1.0), W, H, d_rgba.data_ptr())
    assert L.rvcp_set_demodulation(rt.handle, 1) == abi.RVCP_E_INVALID
    rt.wait()
    assert rt.demodulation is False
    rt.demodulation = True
    assert rt.demodulation is True
    rt.demodulation = False


# ---------------------------------------------------------------------------- 3. chains
CW = CH = 32


def chain_pushes(sc):
    """Two frames: the camera at rest, then moved."""
    out = []
    for i, d in enumerate([(0.0, 0.0, 0.0), (60.0, 20.0, 0.0)]):
        cam = cornell_box().camera
        cam.position = (cam.position + np.asarray(d, dtype=f32)).astype(f32)
        out.append(rvcp_amd.push_constant(cam, 20.0 + i))
    return out


@pytest.fixture(scope="module")
def chain():
    """A context with the checker floor uploaded, its own raw frames and texels of the two
    pushes, and the previous camera's view of each frame."""
    sc = checker_floor_scene()
    pushes = chain_pushes(sc)
    rt = rvcp_amd.RayTracer(spp=2)
    rt.upload_scene(sc)
    raw, gbuf = [], []
    d_g = torch.zeros(CW * CH * 32, dtype=torch.uint8, device="cuda")
    for push in pushes:
        raw.append(rt.render_push(push, CW, CH, want_linear=True)[1])
        torch.cuda.synchronize()
        rt.render_gbuffer_async(push, CW, CH, d_g.data_ptr())
        torch.cuda.synchronize()
        gbuf.append(d_g.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(CH, CW).copy())
    views = [None, abi.temporal_view(pushes[0], CW, CH)]
    table = A.albedo_table(sc.aligned_materials())
    seen = set(np.unique(gbuf[0]["material"][R.filterable(gbuf[0])]).tolist())
    assert {len(table) - 2, len(table) - 1} <= seen               # both checker materials are seen
    yield dict(rt=rt, pushes=pushes, raw=raw, gbuf=gbuf, views=views, table=table)
    rt.close()


def gpu_denoise(rt, c, g, dp):
    H, W = c.shape[:2]
    d_c, d_g, d_out = dev(c), dev(g), blank(W * H * 12)
    torch.cuda.synchronize()
    rt.denoise_async(d_c.data_ptr(), d_g.data_ptr(), W, H, d_out.data_ptr(), 0, dp)
    rt.denoise_wait()
    return floats(d_out, H, W, 3)


def gpu_temporal(rt, c, g, hist, view, tp):
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(a) for a in hist] if hist else None
    d_out, d_len = blank(W * H * 12), blank(W * H * 4)
    torch.cuda.synchronize()
    pp = [t.data_ptr() for t in d_prev] if d_prev else [0, 0, 0]
    rt.temporal_accumulate_async(view if hist else None, d_c.data_ptr(), d_g.data_ptr(), pp[0],
                                 pp[1], pp[2], W, H, d_out.data_ptr(), d_len.data_ptr(), 0, tp)
    rt.temporal_wait()
    return floats(d_out, H, W, 3), d_len.cpu().numpy().view(np.uint32).reshape(H, W)


def gpu_svgf(rt, c, g, hist, view, tp, sp):
    """rvcp_svgf_accumulate_async then rvcp_svgf_filter_async without an RGBA8 store."""
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(a) for a in hist] if hist else None
    d_a, d_n, d_m = blank(W * H * 12), blank(W * H * 4), blank(W * H * 8)
    d_out, d_var = blank(W * H * 12), blank(W * H * 4)
    torch.cuda.synchronize()
    pp = [t.data_ptr() for t in d_prev] if d_prev else [0, 0, 0, 0]
    rt.svgf_accumulate_async(view if hist else None, d_c.data_ptr(), d_g.data_ptr(), pp[0], pp[1],
                             pp[2], pp[3], W, H, d_a.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), 0,
                             tp, sp)
    rt.svgf_filter_async(d_a.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), d_g.data_ptr(), W, H,
                         d_out.data_ptr(), d_var.data_ptr(), 0, 0, sp)
    rt.svgf_wait()
    return (floats(d_out, H, W, 3), floats(d_var, H, W),
            floats(d_a, H, W, 3), d_n.cpu().numpy().view(np.uint32).reshape(H, W),
            floats(d_m, H, W, 2))


def render_denoised_push(rt, push, dp):
    """rvcp_render_denoised for an explicit push constant: (rgba, linear)."""
    push = np.ascontiguousarray(push)
    rgba = np.empty((CH, CW, 4), dtype=np.uint8)
    lin = np.empty((CH, CW, 3), dtype=np.float32)
    rc = abi.load().rvcp_render_denoised(rt.handle, abi.ptr(push), CW, CH, abi.ptr(dp), abi.ptr(rgba),
                                         abi.ptr(lin), None, None)
    assert rc == abi.RVCP_OK, rc
    return rgba, lin


def test_render_svgf_chain_with_the_switch(chain):
    rt, tp, sp = chain["rt"], abi.make_temporal_params(), abi.make_svgf_params()
    ref = A.SvgfChain(chain["table"], tp, sp)
    rt.demodulation = True
    hist = None
    try:
        for i, push in enumerate(chain["pushes"]):
            raw, g, view = chain["raw"][i], chain["gbuf"][i], chain["views"][i]
            rgba, lin, var, n = rt.render_svgf_push(push, CW, CH, tp, sp, want_linear=True,
                                                    want_variance=True, want_history=True)
            # the library's own stateless composition
            e = gpu_demodulate(rt, raw, g)
            out, s_var, a, s_n, m = gpu_svgf(rt, e, g, hist, view, tp, sp)
            s_lin, s_rgba = gpu_remodulate(rt, out, g)
            hist = (a, g, s_n, m)
            assert_same(lin, s_lin, f"frame {i} colour")
            assert_same(var, s_var, f"frame {i} variance")
            assert np.array_equal(rgba, s_rgba) and np.array_equal(n, s_n), i
            # ... equals the restatement's chain
            want, want_var, want_n = ref.frame(raw, g, view)
            assert_same(s_lin, want, f"frame {i} colour vs restatement")
            assert_same(s_var, want_var, f"frame {i} variance vs restatement")
            assert np.array_equal(s_n, want_n) and np.array_equal(s_rgba, R.gamma_rgba(want)), i
        assert (n == 2).any()                                 # the moved frame kept some history
    finally:
        rt.demodulation = False


def test_render_denoised_chain_with_the_switch(chain):
    rt, dp = chain["rt"], abi.make_denoise_params()
    rt.demodulation = True
    try:
        for i, push in enumerate(chain["pushes"]):
            raw, g = chain["raw"][i], chain["gbuf"][i]
            rgba, lin = render_denoised_push(rt, push, dp)
            e = gpu_demodulate(rt, raw, g)
            s_lin, s_rgba = gpu_remodulate(rt, gpu_denoise(rt, e, g, dp), g)
            assert_same(lin, s_lin, f"frame {i} colour")
            assert np.array_equal(rgba, s_rgba), i
            want = A.denoise_chain(raw, g, chain["table"], dp)
            assert_same(s_lin, want, f"frame {i} colour vs restatement")
            assert np.array_equal(s_rgba, R.gamma_rgba(want)), i
    finally:
        rt.demodulation = False


@pytest.mark.parametrize("denoise", [True, False], ids=["denoise", "plain"])
def test_render_temporal_chain_with_the_switch(chain, denoise):
    rt, tp = chain["rt"], abi.make_temporal_params()
    dp = abi.make_denoise_params() if denoise else None
    ref = A.TemporalChain(chain["table"], tp, dp)
    rt.demodulation = True
    hist = None
    try:
        for i, push in enumerate(chain["pushes"]):
            raw, g, view = chain["raw"][i], chain["gbuf"][i], chain["views"][i]
            rgba, lin, n = rt.render_temporal_push(push, CW, CH, tp, dp, want_linear=True,
                                                   want_history=True)
            e = gpu_demodulate(rt, raw, g)
            a, s_n = gpu_temporal(rt, e, g, hist, view, tp)
            hist = (a, g, s_n)
            s_lin, s_rgba = gpu_remodulate(rt, gpu_denoise(rt, a, g, dp) if denoise else a, g)
            assert_same(lin, s_lin, f"frame {i} colour")
            assert np.array_equal(rgba, s_rgba) and np.array_equal(n, s_n), i
            want, want_n = ref.frame(raw, g, view)
            assert_same(s_lin, want, f"frame {i} colour vs restatement")
            assert np.array_equal(s_n, want_n) and np.array_equal(s_rgba, R.gamma_rgba(want)), i
    finally:
        rt.demodulation = False


# ---------------------------------------------------------------------------- 4. the switch
def all_chains(rt, push, time):
    """One frame of each chain: a tuple of arrays."""
    dp = abi.make_denoise_params()
    out = rt.render_svgf_push(push, CW, CH, want_linear=True, want_variance=True, want_history=True)
    out += rt.render_temporal_push(push, CW, CH, None, dp, want_linear=True, want_history=True)
    out += rt.render_denoised(CW, CH, time, dp, want_linear=True)
    return out


def test_switch_on_and_off_again_equals_a_fresh_context(chain):
    rt, push = chain["rt"], chain["pushes"][0]
    rt.svgf_reset()
    rt.temporal_reset()
    rt.demodulation = True
    all_chains(rt, push, 20.0)
    rt.demodulation = False
    got = [all_chains(rt, push, 20.0 + k) for k in range(2)]
    with rvcp_amd.RayTracer(spp=2) as fresh:
        fresh.upload_scene(checker_floor_scene())
        want = [all_chains(fresh, push, 20.0 + k) for k in range(2)]
    for k in range(2):
        for a, b in zip(got[k], want[k]):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8)), k


def test_toggling_drops_the_histories_and_the_same_value_keeps_them(chain):
    rt, push = chain["rt"], chain["pushes"][0]
    fresh = R.filterable(chain["gbuf"][0]).astype(np.uint32)

    def lens():
        s = rt.render_svgf_push(push, CW, CH, want_history=True)[1]
        t = rt.render_temporal_push(push, CW, CH, want_history=True)[1]
        return s, t

    rt.svgf_reset()
    rt.temporal_reset()
    try:
        assert all(np.array_equal(n, fresh) for n in lens())
        assert all(np.array_equal(n, 2 * fresh) for n in lens())
        rt.demodulation = False                                # the value it has: nothing happens
        assert all(np.array_equal(n, 3 * fresh) for n in lens())
        rt.demodulation = True                                 # off -> on
        assert all(np.array_equal(n, fresh) for n in lens())
        rt.demodulation = True
        assert all(np.array_equal(n, 2 * fresh) for n in lens())
        rt.demodulation = False                                # on -> off
        assert all(np.array_equal(n, fresh) for n in lens())
    finally:
        rt.demodulation = False


# ---------------------------------------------------------------------------- 5. white scene
def test_white_scene_renders_identical_bytes_with_the_switch():
    """Every Lambertian albedo (1, 1, 1): c / 1 and e * 1 are exact, so all three chains give the
    same bytes with the switch on and off."""
    sc = white_scene()
    push = sc.push_constant(9.0)
    frames = {}
    for on in (False, True):
        with rvcp_amd.RayTracer(spp=2) as rt:
            rt.upload_scene(sc)
            rt.demodulation = on
            frames[on] = [all_chains(rt, push, 9.0) for _ in range(2)]
    for k in range(2):
        for a, b in zip(frames[False][k], frames[True][k]):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                  np.ascontiguousarray(b).view(np.uint8)), k
