"""Temporal reprojection and accumulation on the GPU: every accumulated float
and every history length bit-identical to the numpy restatement (tests/temporal_ref.py), the
RGBA8 store equal to oracle.gamma_u8 of those floats, the stateful chain of rvcp_render_temporal
against the restatement fed the same context's own frames and texels, the quality gate, the
argument checks (every rejected call is rejected on the host before any launch) and the
interactive loop."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
import oracle as O
import rvcp_amd
from rvcp_amd import abi
from rvcp_amd import interactive as I

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    """A numpy array's bytes in a torch device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.fixture(scope="module")
def tracers():
    """One scene-less context per unorm_rule: the accumulation needs no scene."""
    rts = [rvcp_amd.RayTracer(unorm_rule=rule) for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST)]
    yield rts
    for rt in rts:
        rt.close()


def gpu_accumulate(rt, c, g, pc, pg, pl, view, params, want_rgba=True):
    """rvcp_temporal_accumulate_async on device tensors (the context's own stream);
    (floats, lengths, rgba).  The outputs start from a pattern no result has."""
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(a) for a in (pc, pg, pl)] if pc is not None else None
    d_out = torch.full((W * H * 12,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((W * H * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    d_rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pp = [t.data_ptr() for t in d_prev] if d_prev else [0, 0, 0]
    rt.temporal_accumulate_async(view, d_c.data_ptr(), d_g.data_ptr(), pp[0], pp[1], pp[2], W, H,
                                 d_out.data_ptr(), d_len.data_ptr(),
                                 d_rgba.data_ptr() if want_rgba else 0, params)
    assert rt.temporal_wait() >= 0.0
    return (d_out.cpu().numpy().view(np.float32).reshape(H, W, 3),
            d_len.cpu().numpy().view(np.uint32).reshape(H, W),
            d_rgba.cpu().numpy().reshape(H, W, 4))


# ---------------------------------------------------------------------------- 1. kernel parity
SIZES = [(67, 45), (130, 3), (70, 5), (8, 8), (1, 1), (64, 8), (65, 9)]   # .. on / past the tile
PARAM_SETS = {"max_history_1": dict(max_history=1),
              "alpha_min_0": dict(alpha_min=0.0, max_history=40, normal_min=0.8, sigma_plane=0.25)}


@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("mode", ["identity", "reprojection", "no_history"])
@pytest.mark.parametrize("W,H", SIZES)
def test_accumulate_matches_numpy_restatement(tracers, W, H, mode, pname):
    params = abi.make_temporal_params(**PARAM_SETS[pname])
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed=W * 1000 + H, identity=mode == "identity",
                                              p=params)
    if W * H == 1:
        g["face"], g["material"] = 7, g["material"] & np.uint32(3)  # the single pixel is filterable
    else:
        assert R.filterable(g).any() and not R.filterable(g).all()
    if mode == "no_history":
        pc = pg = pl = None
    v = None if mode == "identity" else view
    want, want_len = T.accumulate(c, g, pc, pg, pl, v, params)
    for rule, rt in enumerate(tracers):
        got, got_len, rgba = gpu_accumulate(rt, c, g, pc, pg, pl, v, params)
        diff = np.any(bits(got) != bits(want), axis=-1)
        assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ (rule {rule})"
        assert np.array_equal(got_len, want_len), rule
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


def test_accumulate_default_params_and_no_rgba(tracers):
    """params = NULL takes rvcp_temporal_params_default; d_rgba8_out is optional."""
    c, g, pc, pg, pl, view = T.synthetic_case(33, 17, seed=11)
    want, want_len = T.accumulate(c, g, pc, pg, pl, view, abi.make_temporal_params())
    got, got_len, rgba = gpu_accumulate(tracers[0], c, g, pc, pg, pl, view, None, want_rgba=False)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_len, want_len)
    assert not rgba.any()


# ---------------------------------------------------------------------------- 2. stateful chain
CHAIN_W, CHAIN_H = 37, 23
MOVES = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (60.0, 20.0, 0.0), (60.0, 20.0, 0.0), (35.0, -15.0, 40.0)]


def chain_pushes():
    """Five frames: two static, a move, a static one, a second move; a time seed each."""
    out = []
    for i, d in enumerate(MOVES):
        sc = rvcp_amd.Scene.default()
        sc.camera.position = (sc.camera.position + np.asarray(d, dtype=f32)).astype(f32)
        out.append(sc.push_constant(20.0 + i))
    return out


@pytest.fixture(scope="module")
def chain(cornell):
    """The chain's inputs from one context (its own render_push frames and render_gbuffer_async
    texels for the five pushes) and the restatement's accumulated frames over them."""
    W, H = CHAIN_W, CHAIN_H
    pushes = chain_pushes()
    rt = rvcp_amd.RayTracer(spp=2)
    rt.upload_scene(cornell)
    raw, gbuf = [], []
    d_g = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    for push in pushes:
        raw.append(rt.render_push(push, W, H, want_linear=True)[1])
        torch.cuda.synchronize()
        rt.render_gbuffer_async(push, W, H, d_g.data_ptr())
        torch.cuda.synchronize()
        gbuf.append(d_g.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W).copy())
    p = abi.make_temporal_params()
    acc, lens = [], []
    for i in range(len(pushes)):
        if i == 0:
            a, n = T.accumulate(raw[0], gbuf[0], None, None, None, None, p)
        else:
            same = pushes[i]["camera"].tobytes() == pushes[i - 1]["camera"].tobytes()
            view = None if same else abi.temporal_view(pushes[i - 1], W, H)
            a, n = T.accumulate(raw[i], gbuf[i], acc[-1], gbuf[i - 1], lens[-1], view, p)
        acc.append(a)
        lens.append(n)
    # the chain exercises what it is meant to: histories that continue, that are reprojected
    # (with rejected taps) and that restart
    filt = [R.filterable(g) for g in gbuf]
    assert np.array_equal(lens[1], 2 * filt[1].astype(np.uint32))
    assert (lens[2] == 3).any() and (lens[2][filt[2]] == 1).any()
    assert (lens[4] == 5).any() and (lens[4][filt[4]] == 1).any()
    yield dict(rt=rt, pushes=pushes, raw=raw, gbuf=gbuf, acc=acc, lens=lens, params=p)
    rt.close()


def test_render_temporal_chain(chain):
    rt, W, H = chain["rt"], CHAIN_W, CHAIN_H
    rt.temporal_reset()
    for i, push in enumerate(chain["pushes"]):
        rgba, lin, hist = rt.render_temporal_push(push, W, H, chain["params"], want_linear=True,
                                                  want_history=True)
        assert rt.last_temporal_ms > 0.0 and rt.last_denoise_ms == 0.0
        assert int(rt.last_stats["samples"]) == W * H * 2
        assert np.array_equal(hist, chain["lens"][i]), i
        assert np.array_equal(bits(lin), bits(chain["acc"][i])), i
        assert np.array_equal(rgba, R.gamma_rgba(chain["acc"][i])), i
    # a plain render on the same context is untouched by the history
    again = rt.render_push(chain["pushes"][0], W, H, want_linear=True)[1]
    assert np.array_equal(bits(again), bits(chain["raw"][0]))


def test_render_temporal_chain_with_the_spatial_pass(chain):
    """RVCP_TEMPORAL_DENOISE filters what is shown; the history keeps the unfiltered frame."""
    rt, W, H = chain["rt"], CHAIN_W, CHAIN_H
    dparams = abi.make_denoise_params(iterations=3, normal_power_log2=5, sigma_color=1.0)
    rt.temporal_reset()
    for i, push in enumerate(chain["pushes"]):
        rgba, lin, hist = rt.render_temporal_push(push, W, H, chain["params"], dparams,
                                                  want_linear=True, want_history=True)
        assert rt.last_temporal_ms > 0.0 and rt.last_denoise_ms > 0.0
        want = R.denoise_params(chain["acc"][i], chain["gbuf"][i], dparams)
        assert np.array_equal(hist, chain["lens"][i]), i
        assert np.array_equal(bits(lin), bits(want)), i
        assert np.array_equal(rgba, R.gamma_rgba(want)), i


def test_history_restarts(chain, cornell):
    rt, W, H = chain["rt"], CHAIN_W, CHAIN_H
    push, p = chain["pushes"][0], chain["params"]
    fresh = R.filterable(chain["gbuf"][0]).astype(np.uint32)

    def frame(w=W, h=H):
        _, lin, hist = rt.render_temporal_push(push, w, h, p, want_linear=True, want_history=True)
        return lin, hist

    rt.temporal_reset()
    lin, hist = frame()
    assert np.array_equal(hist, fresh) and np.array_equal(bits(lin), bits(chain["raw"][0]))
    assert np.array_equal(frame()[1], 2 * fresh)
    rt.temporal_reset()                                   # 1. rvcp_temporal_reset
    lin, hist = frame()
    assert np.array_equal(hist, fresh) and np.array_equal(bits(lin), bits(chain["raw"][0]))
    assert np.array_equal(frame()[1], 2 * fresh)
    assert frame(W - 5, H)[1].max() == 1                  # 2. a size change, there ...
    assert frame(W - 5, H)[1].max() == 2
    assert np.array_equal(frame()[1], fresh)              # ... and back
    assert np.array_equal(frame()[1], 2 * fresh)
    rt.upload_scene(cornell)                              # 3. a scene upload
    lin, hist = frame()
    assert np.array_equal(hist, fresh) and np.array_equal(bits(lin), bits(chain["raw"][0]))


# ---------------------------------------------------------------------------- 3. quality
def test_quality_gate_through_render_temporal(cornell):
    """The CPU gate (test_temporal_cpu) on the GPU's own frames: static camera, Cornell 64^2,
    SPP = 4, 8 frames at the defaults against the first raw frame."""
    W = H = 64
    mask, ref = R.filterable(R.cornell_gbuffer(W, H)), R.cornell_reference(W, H)
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        first = rt.render(W, H, T.QUALITY_SEEDS[0], want_linear=True)[1]
        for t in T.QUALITY_SEEDS:
            _, lin, hist = rt.render_temporal(W, H, t, want_linear=True, want_history=True)
    assert np.array_equal(hist, 8 * mask.astype(np.uint32))
    before, after = R.rmse(first, ref, mask), R.rmse(lin, ref, mask)
    print(f"rmse first raw {before:.4f} accumulated {after:.4f} ratio {after / before:.4f} "
          f"gate {T.QUALITY_GATE:.4f}")
    assert after <= T.QUALITY_GATE * before


# ---------------------------------------------------------------------------- 4. API
def test_api_argument_checks(cornell, cornell_arrays):
    L = abi.load()
    W = H = 16
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed=5)
    npx = W * H
    d_c, d_g, d_pc, d_pg, d_pl = dev(c), dev(g), dev(pc), dev(pg), dev(pl)
    d_out = torch.zeros(npx * 12 + 64, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(npx * 4 + 64, dtype=torch.uint8, device="cuda")
    d_rgba = torch.zeros(npx * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P = lambda a: ctypes.c_void_p(a) if a else None       # noqa: E731
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    ok = abi.make_temporal_params()
    E = abi.RVCP_E_INVALID
    with rvcp_amd.RayTracer(spp=2) as rt:                 # no scene uploaded
        h = rt.handle
        base = dict(view=view, cur=d_c.data_ptr(), cur_g=d_g.data_ptr(), prev=d_pc.data_ptr(),
                    prev_g=d_pg.data_ptr(), prev_len=d_pl.data_ptr(), w=W, h=H, params=ok,
                    out=d_out.data_ptr(), out_len=d_len.data_ptr(), rgba=d_rgba.data_ptr())

        def call(**kw):
            a = dict(base, **kw)
            return L.rvcp_temporal_accumulate_async(
                h, abi.ptr(a["view"]), P(a["cur"]), P(a["cur_g"]), P(a["prev"]), P(a["prev_g"]),
                P(a["prev_len"]), a["w"], a["h"], abi.ptr(a["params"]), P(a["out"]),
                P(a["out_len"]), P(a["rgba"]), None)
        for name in ("cur", "cur_g", "out", "out_len", "w", "h"):         # NULL or zero
            assert call(**{name: 0}) == E, name
        for name in ("prev", "prev_g", "prev_len"):                       # a partial triple
            assert call(**{name: 0}) == E, name
            rest = {k: 0 for k in ("prev", "prev_g", "prev_len") if k != name}
            assert call(**rest) == E, name
        assert b"together" in L.rvcp_last_error(h)
        # outputs over inputs (taps read neighbours: in place is wrong) and over each other
        for kw in (dict(out=base["cur"]), dict(out=base["prev"]), dict(out=base["prev"] + 12),
                   dict(out=base["cur_g"]), dict(out=base["prev_g"] + 32 * npx - 4),
                   dict(out_len=base["prev_len"]), dict(out_len=base["prev_len"] + 4 * npx - 4),
                   dict(out_len=base["cur"]), dict(rgba=base["cur_g"]), dict(rgba=base["prev"]),
                   dict(rgba=base["out"]), dict(out_len=base["out"] + 12 * npx - 4)):
            assert call(**kw) == E, kw
            assert b"overlap" in L.rvcp_last_error(h)
        for kw in (dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=float("nan")),
                   dict(max_history=0), dict(max_history=65536), dict(sigma_plane=0.0),
                   dict(sigma_plane=-1.0), dict(sigma_plane=float("nan")), dict(normal_min=-1.5),
                   dict(normal_min=1.5), dict(normal_min=float("nan"))):
            assert call(params=abi.make_temporal_params(**kw)) == E, kw
        assert L.rvcp_temporal_wait(h, None) == E          # nothing was enqueued
        assert not d_out.cpu().numpy().any() and not d_len.cpu().numpy().any()
        # rvcp_render_temporal
        out = np.zeros((H, W, 4), np.uint8)

        def render(push_=push, w=W, hh=H, flags=0, rgba=out):
            return L.rvcp_render_temporal(h, abi.ptr(push_), w, hh, None, flags, None,
                                          abi.ptr(rgba), None, None, None, None, None)
        assert render(push_=None) == E and render(w=0) == E and render(hh=0) == E
        assert render(rgba=None) == E and render(flags=2) == E
        assert render() == abi.RVCP_E_NO_SCENE
        assert L.rvcp_temporal_reset(h) == abi.RVCP_OK
        # the limits of the ranges are inside them
        edge = abi.make_temporal_params(alpha_min=1.0, max_history=65535, normal_min=-1.0)
        assert call(params=edge) == abi.RVCP_OK
        assert rt.temporal_wait() >= 0.0
        want, want_len = T.accumulate(c, g, pc, pg, pl, view, edge)
        got = d_out.cpu().numpy()[:npx * 12].view(np.float32).reshape(H, W, 3)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(d_len.cpu().numpy()[:npx * 4].view(np.uint32).reshape(H, W), want_len)
        # after all of that a plain render is still bit-exact against the oracle
        rt.upload_scene(cornell)
        rgba, lin = rt.render(32, 32, 123.0, want_linear=True)
    o_lin, o_rgba, _ = O.render(cornell_arrays, cornell.push_constant(123.0),
                                abi.make_config(spp=2), 32, 32)
    assert np.array_equal(rgba, o_rgba) and np.array_equal(bits(lin), bits(o_lin))


@pytest.mark.parametrize("kw", [dict(integrator=abi.INTEGRATOR_LEGACY), dict(n_gpus=2)])
def test_render_temporal_unsupported_contexts(cornell, kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(cornell)
        with pytest.raises(abi.RvcpError) as e:
            rt.render_temporal(16, 16, 1.0)
        assert e.value.code == abi.RVCP_E_UNSUPPORTED


def test_bad_filter_parameters_midway_drain_the_chain(cornell):
    """A call whose filter is rejected after the render and the temporal step were enqueued waits
    for what it enqueued, leaves nothing pending and drops the history."""
    L = abi.load()
    W = H = 16
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        assert rt.render_temporal(W, H, 1.0, want_history=True)[1].max() == 1
        assert rt.render_temporal(W, H, 2.0, want_history=True)[1].max() == 2
        with pytest.raises(abi.RvcpError) as e:
            rt.render_temporal(W, H, 3.0, denoise=abi.make_denoise_params(iterations=9))
        assert e.value.code == abi.RVCP_E_INVALID and "denoise iterations" in str(e.value)
        for wait in (L.rvcp_temporal_wait, L.rvcp_denoise_wait):      # the chain drained its step
            assert wait(rt.handle, None) == abi.RVCP_E_INVALID
            assert b"in flight" in L.rvcp_last_error(rt.handle)
        rt.render(W, H, 4.0)                               # nothing is left pending
        assert rt.render_temporal(W, H, 5.0, want_history=True)[1].max() == 1


def test_accumulate_is_ordered_behind_a_pending_render(cornell, cornell_arrays):
    """A render pending on the context is no error: on the same stream the step reads the frame
    and the texels that render and the G-buffer pass leave."""
    W = H = 24
    d_rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    d_lin = torch.zeros(W * H * 12, dtype=torch.uint8, device="cuda")
    d_g = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(W * H * 12, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    push = cornell.push_constant(9.0)
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        rt.render_async(push, W, H, d_rgba.data_ptr(), d_lin.data_ptr())
        rt.render_gbuffer_async(push, W, H, d_g.data_ptr())
        rt.temporal_accumulate_async(None, d_lin.data_ptr(), d_g.data_ptr(), 0, 0, 0, W, H,
                                     d_out.data_ptr(), d_len.data_ptr())
        rt.wait()
        rt.temporal_wait()
    noisy, _, _ = O.render(cornell_arrays, push, abi.make_config(spp=2), W, H)
    g = d_g.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W)
    assert np.array_equal(bits(d_out.cpu().numpy().view(np.float32).reshape(H, W, 3)), bits(noisy))
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32).reshape(H, W),
                          R.filterable(g).astype(np.uint32))


# ---------------------------------------------------------------------------- 5. interactive
def test_run_headless_temporal(tmp_path, cornell_arrays):
    """run_headless(temporal=...) over 4 frames with a scripted key event writes its frames: the
    first (no history yet) is the plain render of its seed, the later ones are accumulated; and
    run_headless() without the argument still renders the raw frame."""
    W, H = 48, 40
    sc = rvcp_amd.Scene.default()
    cfg = abi.make_config(spp=2)
    events = [(2, "key", ("W", True))]
    seed = lambda i: 10.0 + i                              # noqa: E731
    push0 = sc.push_constant(seed(0))
    a, b = tmp_path / "temporal", tmp_path / "plain"
    with rvcp_amd.RayTracer(cfg) as rt:
        rt.upload_scene(sc)
        out = I.run_headless(rt, sc, 4, W, H, events=events, fixed_dt=0.05, time_seed=seed,
                             dump_dir=str(a), on_fps=lambda n: None,
                             temporal=abi.make_temporal_params())
        assert out["camera_moved"] == [False, False, True, True] and len(out["frame_ms"]) == 4
        assert rt.last_temporal_ms > 0.0
        frames = [I.read_ppm(str(a / f"frame_{i:05d}.ppm")) for i in range(4)]
        push3 = sc.push_constant(13.0)                     # where the loop left the camera
        I.run_headless(rt, sc, 1, W, H, fixed_dt=0.05, time_seed=lambda i: 13.0, dump_dir=str(b),
                       on_fps=lambda n: None)
        plain = I.read_ppm(str(b / "frame_00000.ppm"))
    o0 = O.render(cornell_arrays, push0, cfg, W, H)[1]
    o3 = O.render(cornell_arrays, push3, cfg, W, H)[1]
    assert all(f.shape == (H, W, 3) for f in frames)
    assert np.array_equal(frames[0], o0[..., :3])
    assert np.array_equal(plain, o3[..., :3])
    assert not np.array_equal(frames[3], plain)            # accumulated, not the raw frame
