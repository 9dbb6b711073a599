"""Temporal anti-aliasing on the GPU: rvcp_taa_resolve_async bit-identical to
the numpy restatement (tests/taa_ref.py) with no pixel excluded, the fused store equal to
oracle.gamma_u8 of the resolved floats under both unorm_rules, the argument checks (every rejected
call is rejected on the host before any launch), rvcp_render_temporal and rvcp_render_svgf with the
switch on against the library's own stateless composition and against the restatements, the
restarts, the switch off against a context that never heard of TAA, and the two quality gates."""
import ctypes

import numpy as np
import pytest

import albedo_ref as AL
import denoise_ref as R
import svgf_ref as S
import taa_ref as A
import temporal_ref as T
import rvcp_amd
from rvcp_amd import abi
from test_gpu_albedo import (assert_same, bits, blank, dev, floats, gpu_demodulate, gpu_remodulate,
                             gpu_svgf, gpu_temporal)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = np.float32
SEED = 1


@pytest.fixture(scope="module")
def tracers():
    """One scene-less context per unorm_rule: the resolve needs no scene."""
    rts = [rvcp_amd.RayTracer(unorm_rule=rule) for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST)]
    yield rts
    for rt in rts:
        rt.close()


def gpu_resolve(rt, c, g, pr, pl, cv, pv, params, want_rgba=True):
    """rvcp_taa_resolve_async on device tensors (the context's own stream); (floats, lengths,
    rgba).  The outputs start from a pattern no result has."""
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(pr), dev(pl)] if pr is not None else None
    d_out, d_len, d_rgba = blank(W * H * 12), blank(W * H * 4), blank(W * H * 4, 0)
    torch.cuda.synchronize()
    pp = [t.data_ptr() for t in d_prev] if d_prev else [0, 0]
    rt.taa_resolve_async(cv, pv, d_c.data_ptr(), d_g.data_ptr(), pp[0], pp[1], W, H,
                         d_out.data_ptr(), d_len.data_ptr(), d_rgba.data_ptr() if want_rgba else 0,
                         params)
    assert rt.taa_wait() >= 0.0
    return (floats(d_out, H, W, 3), d_len.cpu().numpy().view(np.uint32).reshape(H, W),
            d_rgba.cpu().numpy().reshape(H, W, 4))


# ---------------------------------------------------------------------------- 1. kernel parity
# a ragged last wave and last row of blocks; three waves by one block; a thin frame; one wave;
# one interior pixel; all border; one pixel
SIZES = [(67, 45), (130, 3), (70, 5), (8, 8), (3, 3), (2, 2), (1, 1)]
PARAM_SETS = {"defaults": dict(), "clamp_0": dict(clamp=0), "max_history_1": dict(max_history=1),
              "alpha_min_0": dict(alpha_min=0.0, max_history=40)}


@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("mode", ["no_history", "identity", "reprojection"])
@pytest.mark.parametrize("W,H", SIZES)
def test_resolve_matches_numpy_restatement(tracers, W, H, mode, pname):
    params = abi.make_taa_params(**PARAM_SETS[pname])
    c, g, pr, pl, cv, pv = A.synthetic_case(W, H, SEED, params)
    if mode == "no_history":
        pr = pl = None
    if mode == "identity":
        cv = pv = None
    want, want_len = A.resolve(c, g, pr, pl, cv, pv, params)
    for rule, rt in enumerate(tracers):
        got, got_len, rgba = gpu_resolve(rt, c, g, pr, pl, cv, pv, params)
        diff = np.any(bits(got) != bits(want), axis=-1)
        assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ (rule {rule})"
        assert np.array_equal(got_len, want_len), rule
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


def test_resolve_default_params_no_rgba_and_equal_views(tracers):
    """params = NULL takes rvcp_taa_params_default; d_rgba8_out is optional; two byte-equal view
    records are the identity path (q = p, no resampling)."""
    c, g, pr, pl, cv, pv = A.synthetic_case(33, 17, SEED)
    want, want_len = A.resolve(c, g, pr, pl, cv, pv, A.params())
    got, got_len, rgba = gpu_resolve(tracers[0], c, g, pr, pl, cv, pv, None, want_rgba=False)
    assert_same(got, want, "default parameters")
    assert np.array_equal(got_len, want_len) and not rgba.any()
    ident, ident_len = A.resolve(c, g, pr, pl, None, None, A.params())
    got, got_len, _ = gpu_resolve(tracers[0], c, g, pr, pl, cv, cv.copy(), None)
    assert_same(got, ident, "byte-equal views")
    assert np.array_equal(got_len, ident_len)
    assert np.any(bits(ident) != bits(want))


# ---------------------------------------------------------------------------- 2. API
def test_api_argument_checks(cornell):
    L = abi.load()
    W = H = 16
    c, g, pr, pl, cv, pv = A.synthetic_case(W, H, SEED)
    npx = W * H
    d_c, d_g, d_pr, d_pl = dev(c), dev(g), dev(pr), dev(pl)
    d_out, d_len, d_rgba = blank(npx * 12 + 64), blank(npx * 4 + 64), blank(npx * 4)
    torch.cuda.synchronize()
    P = lambda a: ctypes.c_void_p(a) if a else None       # noqa: E731
    E = abi.RVCP_E_INVALID
    with rvcp_amd.RayTracer(spp=2) as rt:                 # no scene uploaded
        h = rt.handle
        base = dict(cv=cv, pv=pv, cur=d_c.data_ptr(), cur_g=d_g.data_ptr(), prev=d_pr.data_ptr(),
                    prev_len=d_pl.data_ptr(), w=W, h=H, params=abi.make_taa_params(),
                    out=d_out.data_ptr(), out_len=d_len.data_ptr(), rgba=d_rgba.data_ptr())

        def call(**kw):
            a = dict(base, **kw)
            return L.rvcp_taa_resolve_async(
                h, abi.ptr(a["cv"]), abi.ptr(a["pv"]), P(a["cur"]), P(a["cur_g"]), P(a["prev"]),
                P(a["prev_len"]), a["w"], a["h"], abi.ptr(a["params"]), P(a["out"]),
                P(a["out_len"]), P(a["rgba"]), None)
        for name in ("cur", "cur_g", "out", "out_len", "w", "h"):         # NULL or zero
            assert call(**{name: 0}) == E, name
        assert call(w=1 << 16, h=1 << 15) == E                            # W * H = 2^31
        for name in ("prev", "prev_len"):                                 # a partial history
            assert call(**{name: 0}) == E, name
            assert b"together" in L.rvcp_last_error(h)
        for name in ("cv", "pv"):                                         # a partial view pair
            assert call(**{name: None}) == E, name
        # outputs over inputs (taps and the box read neighbours) and over each other
        for kw in (dict(out=base["cur"]), dict(out=base["prev"]), dict(out=base["prev"] + 12),
                   dict(out=base["cur_g"]), dict(out=base["cur_g"] + 32 * npx - 4),
                   dict(out_len=base["prev_len"]), dict(out_len=base["prev_len"] + 4 * npx - 4),
                   dict(out_len=base["cur"]), dict(rgba=base["cur_g"]), dict(rgba=base["prev"]),
                   dict(rgba=base["out"]), dict(out_len=base["out"] + 12 * npx - 4)):
            assert call(**kw) == E, kw
            assert b"overlap" in L.rvcp_last_error(h)
        for kw in (dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=float("nan")),
                   dict(max_history=0), dict(max_history=65536), dict(clamp=2), dict(_pad=1)):
            assert call(params=abi.make_taa_params(**kw)) == E, kw
        assert L.rvcp_taa_wait(h, None) == E               # nothing was enqueued
        for t in (d_out, d_len, d_rgba):                   # ... and nothing was written
            assert np.all(t.cpu().numpy() == 0xA5)
        # the limits of the ranges are inside them, and no scene is needed
        edge = abi.make_taa_params(alpha_min=1.0, max_history=65535)
        assert call(params=edge) == abi.RVCP_OK
        assert rt.taa_wait() >= 0.0
        want, want_len = A.resolve(c, g, pr, pl, cv, pv, edge)
        assert_same(floats(d_out[:npx * 12], H, W, 3), want, "edge parameters")
        assert np.array_equal(d_len.cpu().numpy()[:npx * 4].view(np.uint32).reshape(H, W), want_len)
        # the switch: off by default, refused while a frame is pending
        assert rt.taa is False
        rt.upload_scene(cornell)
        d_f = blank(npx * 4)
        rt.render_async(cornell.push_constant(1.0), W, H, d_f.data_ptr())
        assert L.rvcp_set_taa(h, 1) == E and b"in flight" in L.rvcp_last_error(h)
        rt.wait()
        rt.taa = True
        assert rt.taa is True
        rt.taa_reset()
        rt.taa = False
        assert L.rvcp_get_taa(h, None) == E


# ---------------------------------------------------------------------------- 3. stateful chains
CW, CH = 37, 23
MOVES = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (60.0, 20.0, 0.0), (60.0, 20.0, 0.0), (35.0, -15.0, 40.0)]


def chain_pushes():
    """Five frames: two static, a move, a static one, a second move; a time seed each."""
    out = []
    for i, d in enumerate(MOVES):
        sc = rvcp_amd.Scene.default()
        sc.camera.position = (sc.camera.position + np.asarray(d, dtype=f32)).astype(f32)
        out.append(np.ascontiguousarray(sc.push_constant(20.0 + i)).reshape(()))
    return out


@pytest.fixture(scope="module")
def pair(cornell):
    """Two contexts with the Cornell box: `rt` runs the stateful chains, `rs` the stateless
    steps of the composition."""
    rt, rs = rvcp_amd.RayTracer(spp=2), rvcp_amd.RayTracer(spp=2)
    rt.upload_scene(cornell)
    rs.upload_scene(cornell)
    yield dict(rt=rt, rs=rs, table=AL.albedo_table(cornell.aligned_materials()))
    rt.close()
    rs.close()


def gpu_gbuffer(rs, push, W, H):
    d_g = blank(W * H * 32)
    torch.cuda.synchronize()
    rs.render_gbuffer_async(push, W, H, d_g.data_ptr())
    torch.cuda.synchronize()
    return d_g.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W).copy()


class Composition:
    """The library's own stateless composition of one chain with the switch on, next to the
    restatements' (albedo_ref / svgf_ref / temporal_ref chains, then taa_ref.Chain)."""

    def __init__(self, rs, table, svgf, demod):
        self.rs, self.table, self.svgf, self.demod = rs, table, svgf, demod
        self.tp, self.sp = abi.make_temporal_params(), abi.make_svgf_params()
        self.restart()

    def restart(self):
        self.hist = self.jview = self.res = self.push = self.view = None
        self.counter = 0
        self.ref_taa = A.Chain()
        if self.svgf:
            self.ref = AL.SvgfChain(self.table, self.tp, self.sp) if self.demod else \
                S.Chain(self.tp, self.sp)
        else:
            self.ref = AL.TemporalChain(self.table, self.tp) if self.demod else None
            self.ref_hist = None

    def taa_restart(self):
        """rvcp_taa_reset: the chain's own history stays."""
        self.res, self.counter = None, 0
        self.ref_taa = A.Chain()

    def frame(self, push, W=CW, H=CH):
        """(resolved colour, its RGBA8, history length of the chain) of the next frame."""
        rs = self.rs
        jp = rvcp_amd.taa_jitter_push(push, W, H, rvcp_amd.taa_jitter(self.counter))
        raw = rs.render_push(jp, W, H, want_linear=True)[1]
        g = gpu_gbuffer(rs, jp, W, H)
        c = gpu_demodulate(rs, raw, g) if self.demod else raw
        if self.svgf:
            out, _, a, n, m = gpu_svgf(rs, c, g, self.hist, self.jview, self.tp, self.sp)
            self.hist = (a, g, n, m)
            want = self.ref.frame(raw if self.demod else c, g, self.jview)
            want_final, want_n = want[0], want[2]
        else:
            out, n = gpu_temporal(rs, c, g, self.hist, self.jview, self.tp)
            self.hist = (out, g, n)
            if self.demod:
                want_final, want_n = self.ref.frame(raw, g, self.jview)
            else:
                pc, pg, pl = self.ref_hist if self.ref_hist else (None, None, None)
                want_final, want_n = T.accumulate(c, g, pc, pg, pl, self.jview if pc is not None
                                                  else None, self.tp)
                self.ref_hist = (want_final, g, want_n)
        final = gpu_remodulate(rs, out, g)[0] if self.demod else out
        assert_same(final, want_final, "the chain's final colour vs restatement")
        assert np.array_equal(n, want_n)
        self.jview = abi.temporal_view(jp, W, H)        # the chain's own history always reprojects
        view = abi.temporal_view(push, W, H)
        # no views: without a history, and when the 64 camera bytes equal the previous frame's
        still = self.res is None or push["camera"].tobytes() == self.push["camera"].tobytes()
        pr, pl = self.res if self.res is not None else (None, None)
        res, rlen, rgba = gpu_resolve(rs, final, g, pr, pl, None if still else view,
                                      None if still else self.view, None)
        want_res, want_len = self.ref_taa.step(final, g, push)
        assert_same(res, want_res, "the resolve vs restatement")
        assert np.array_equal(rlen, want_len) and np.array_equal(rgba, R.gamma_rgba(want_res))
        self.res, self.push, self.view = (res, rlen), push, view
        self.counter += 1
        return res, rgba, n


def chain_frame(rt, svgf, push, W=CW, H=CH):
    if svgf:
        rgba, lin, n = rt.render_svgf_push(push, W, H, want_linear=True, want_history=True)
    else:
        rgba, lin, n = rt.render_temporal_push(push, W, H, want_linear=True, want_history=True)
    return lin, rgba, n


@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demodulated"])
@pytest.mark.parametrize("svgf", [False, True], ids=["temporal", "svgf"])
def test_chains_with_the_switch_equal_the_stateless_composition(pair, cornell, svgf, demod):
    rt = pair["rt"]
    comp = Composition(pair["rs"], pair["table"], svgf, demod)
    pushes = chain_pushes()
    rt.demodulation = demod
    rt.taa = True
    try:
        rt.temporal_reset()
        rt.svgf_reset()

        def same(push, what, W=CW, H=CH):
            lin, rgba, n = chain_frame(rt, svgf, push, W, H)
            want, want_rgba, want_n = comp.frame(push, W, H)
            assert_same(lin, want, what)
            assert np.array_equal(rgba, want_rgba) and np.array_equal(n, want_n), what
            return lin, n

        for i, push in enumerate(pushes):
            lin, n = same(push, f"frame {i}")
        assert (n >= 4).any()                             # histories survive the moves
        assert comp.counter == 5 and lin.min() >= 0.0 and lin.max() <= 1.0
        # the restarts: rvcp_taa_reset keeps the chain's own history, the others drop both
        rt.taa_reset()
        comp.taa_restart()
        _, n = same(pushes[4], "after taa_reset")
        assert n.max() >= 5
        (rt.svgf_reset if svgf else rt.temporal_reset)()
        comp.restart()
        _, n = same(pushes[4], "after the chain's reset")
        assert n.max() == 1
        same(pushes[4], "second frame after the reset")
        comp.restart()
        same(pushes[4], "a size change", CW - 5, CH)
        same(pushes[4], "second frame at the new size", CW - 5, CH)
        rt.upload_scene(cornell)
        comp.restart()
        same(pushes[0], "after an upload")
        same(pushes[0], "second frame after the upload")
        rt.taa = True                                      # the value it has: nothing happens
        _, n = same(pushes[0], "third frame, the switch set again")
        assert n.max() == 3
        rt.taa = False
        rt.taa = True                                      # toggled: both histories are dropped
        comp.restart()
        _, n = same(pushes[0], "after toggling")
        assert n.max() == 1
    finally:
        rt.taa = False
        rt.demodulation = False


def test_switch_off_equals_a_context_that_never_heard_of_taa(pair, cornell):
    """Every byte of every output of the three chains and of the plain render, after the switch
    has been on and off again, against a fresh context."""
    rt = pair["rt"]
    pushes = chain_pushes()
    rt.taa = True
    rt.render_temporal_push(pushes[0], CW, CH)
    rt.render_svgf_push(pushes[2], CW, CH)
    rt.taa = False
    dp = abi.make_denoise_params()

    def everything(t):
        out = []
        for push in pushes[1:4]:
            out += list(t.render_temporal_push(push, CW, CH, None, dp, want_linear=True,
                                               want_history=True))
            out += list(t.render_temporal_push(push, CW, CH, want_linear=True, want_history=True))
            out += list(t.render_svgf_push(push, CW, CH, want_linear=True, want_variance=True,
                                           want_history=True))
            out += list(t.render_push(push, CW, CH, want_linear=True))
        return out

    with rvcp_amd.RayTracer(spp=2) as fresh:
        fresh.upload_scene(cornell)
        want = everything(fresh)
    got = everything(rt)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


FAILED_CHAINS = [(False, False), (True, False), (False, True)]       # svgf, demod
FAILED_IDS = ["temporal", "svgf", "temporal-demodulated"]


def failed_chain_restarts(cornell, svgf, demod, switch, W, H):
    """Context A renders two frames and fails midway in the third, on bad filter parameters behind
    the render; its frames at t4 and t5 must then be, byte for byte, those of a fresh context B
    that renders nothing else: the failure drops the chain's history and the resolve state, and
    the jitter sequence starts over.  switch(rt) sets the switch under test."""
    bad_d, bad_s = abi.make_denoise_params(iterations=9), abi.make_svgf_params(iterations=9)

    def frame(rt, t, bad=False):
        if svgf:
            return rt.render_svgf(W, H, t, svgf=bad_s if bad else None, want_linear=True)
        return rt.render_temporal(W, H, t, denoise=bad_d if bad else abi.make_denoise_params(),
                                  want_linear=True)

    def context():
        rt = rvcp_amd.RayTracer(spp=2)
        rt.upload_scene(cornell)
        rt.demodulation = demod
        switch(rt)
        return rt

    with context() as a, context() as b:
        frame(a, 1.0)
        frame(a, 2.0)
        with pytest.raises(abi.RvcpError) as e:
            frame(a, 3.0, bad=True)
        assert e.value.code == abi.RVCP_E_INVALID and "iterations" in str(e.value)
        for t in (4.0, 5.0):
            (rgba, lin), (want_rgba, want_lin) = frame(a, t), frame(b, t)
            assert rgba.shape == (H, W, 4) and lin.shape == (H, W, 3)
            assert rgba.tobytes() == want_rgba.tobytes() and lin.tobytes() == want_lin.tobytes(), t


@pytest.mark.parametrize("svgf,demod", FAILED_CHAINS, ids=FAILED_IDS)
def test_a_failed_chain_drops_the_taa_state_and_restarts_the_jitter(cornell, svgf, demod):
    def switch(rt):
        rt.taa = True
    failed_chain_restarts(cornell, svgf, demod, switch, 16, 16)


# ---------------------------------------------------------------------------- 4. quality
def test_anti_aliasing_gate_64sq_on_gpu_gbuffers(pair, cornell):
    """The CPU gate (test_taa_cpu) at 64 x 64 on the library's own G-buffers, with the resolved
    frame of the last step computed by the kernel as well."""
    W = H = 64
    rs = pair["rs"]
    base = np.ascontiguousarray(cornell.push_constant(0.0)).reshape(())
    mats = cornell.aligned_materials()
    r = A.aa_gate(W, H, base, mats, lambda push, w, h: gpu_gbuffer(rs, push, w, h))
    print("\nTAA gate 64x64 (GPU G-buffers):", r)
    # the library's jitter is the restatement's, and its resolve the restatement's, frame by frame
    res = None
    ref = A.Chain()
    for i in range(A.GATE_FRAMES):
        jp = rvcp_amd.taa_jitter_push(base, W, H, rvcp_amd.taa_jitter(i))
        assert np.asarray(jp).tobytes() == A.jittered_push(base, H, i).tobytes(), i
        g = gpu_gbuffer(rs, jp, W, H)
        c = A.flat_shade(g, mats)
        out, ln, _ = gpu_resolve(rs, c, g, res[0] if res else None, res[1] if res else None, None,
                                 None, None)
        want, want_len = ref.step(c, g, base)
        assert_same(out, want, f"gate frame {i}")
        assert np.array_equal(ln, want_len)
        res = (out, ln)
    assert r["n_edge"] >= 400
    assert r["ratio"] <= A.gate(A.RATIO_MEASURED[(64, 64)])
    assert r["nonedge_resolved"] < r["edge_resolved"]


def path_gate_measure(cornell):
    """(edge rmse off, edge rmse on, all-pixel rmse off, all-pixel rmse on) of rvcp_render_svgf
    at 64 x 64, SPP 4, after 16 frames, against box4 of the clamped plain render at 256 x 256,
    SPP 128."""
    W = H = 64
    with rvcp_amd.RayTracer(spp=128) as hi:
        hi.upload_scene(cornell)
        truth = A.box4(A.sat(hi.render(4 * W, 4 * H, 77.0, want_linear=True)[1]))
        g_hi = gpu_gbuffer(hi, cornell.push_constant(0.0), 4 * W, 4 * H)
    edge = A.edge_pixels(g_hi["face"])
    out = {}
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        for on in (False, True):
            rt.taa = on
            for i in range(A.GATE_FRAMES):
                lin = rt.render_svgf(W, H, 5.0 + i, want_linear=True)[1]
            d = A.sat(lin).astype(np.float64) - truth
            out[on] = (float(np.sqrt(np.mean(d[edge] ** 2))), float(np.sqrt(np.mean(d ** 2))))
    return out[False][0], out[True][0], out[False][1], out[True][1], int(edge.sum())


def test_path_traced_gate_render_svgf_64sq(cornell):
    """The switch on against the switch off through rvcp_render_svgf: the edge pixels' distance
    to the supersampled truth must fall to PATH_MEASURED's ratio plus a quarter of the distance to
    1, and the all-pixel RMSE must not rise."""
    e_off, e_on, a_off, a_on, n_edge = path_gate_measure(cornell)
    print(f"\nTAA path-traced gate: {n_edge} edge pixels, edge rmse off {e_off:.4f} on {e_on:.4f} "
          f"ratio {e_on / e_off:.4f}; all-pixel rmse off {a_off:.4f} on {a_on:.4f}")
    m_off, m_on = A.PATH_MEASURED[0], A.PATH_MEASURED[1]
    assert e_on / e_off <= A.gate(m_on / m_off)
    assert a_on <= a_off
