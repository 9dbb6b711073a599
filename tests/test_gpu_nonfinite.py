"""The non-finite contract of the post-process kernels on the GPU: with NaNs,
infinities, signed zeros, subnormals, huge values and zero normals salted into every float field,
each kernel still gives the bits of its numpy restatement (NaN equal to NaN); a poisoned texel is
treated exactly as a MISS texel (two launches compared, no restatement involved); one bad sample
does not outlive its frame in the SVGF loop; and a scene whose bounces produce non-finite samples
goes through the library's chains as through the restatements, its bad pixels staying where they
fell."""
import numpy as np
import pytest

import albedo_ref as AL
import denoise_ref as R
import nonfinite as N
import svgf_ref as S
import taa_ref as TA
import taau_ref as TU
import temporal_ref as T
import rvcp_amd
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
W0, H0 = 67, 45                     # ragged against the 32 x 8 and the 64 x 4 tiles, several blocks
SHARE = 0.03


def dev(a):
    """A numpy array's bytes in a torch device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def blank(nbytes, fill=0xA5):
    """An output buffer that starts from a pattern no result has."""
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def floats(t, *shape):
    return t.cpu().numpy().view(np.float32).reshape(*shape)


def words(t, *shape):
    return t.cpu().numpy().view(np.uint32).reshape(*shape)


def count(mask):
    return int(np.count_nonzero(mask))


@pytest.fixture(scope="module")
def tracers():
    """One scene-less context per unorm_rule: the stateless steps need no scene."""
    rts = [rvcp_amd.RayTracer(unorm_rule=rule) for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST)]
    yield rts
    for rt in rts:
        rt.close()


# ---------------------------------------------------------------------------- launches
def gpu_denoise(rt, c, g, params):
    H, W = c.shape[:2]
    d_in, d_g = dev(c), dev(g)
    d_out, d_rgba = blank(W * H * 12), blank(W * H * 4, 0)
    torch.cuda.synchronize()
    rt.denoise_async(d_in.data_ptr(), d_g.data_ptr(), W, H, d_out.data_ptr(), d_rgba.data_ptr(),
                     params)
    assert rt.denoise_wait() >= 0.0
    return floats(d_out, H, W, 3), d_rgba.cpu().numpy().reshape(H, W, 4)


def gpu_temporal(rt, c, g, pc, pg, pl, view, params):
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(a) for a in (pc, pg, pl)]
    d_out, d_len, d_rgba = blank(W * H * 12), blank(W * H * 4), blank(W * H * 4, 0)
    torch.cuda.synchronize()
    rt.temporal_accumulate_async(view, d_c.data_ptr(), d_g.data_ptr(), d_prev[0].data_ptr(),
                                 d_prev[1].data_ptr(), d_prev[2].data_ptr(), W, H,
                                 d_out.data_ptr(), d_len.data_ptr(), d_rgba.data_ptr(), params)
    assert rt.temporal_wait() >= 0.0
    return floats(d_out, H, W, 3), words(d_len, H, W), d_rgba.cpu().numpy().reshape(H, W, 4)


def gpu_svgf_accumulate(rt, c, g, pc, pg, pl, pm, view, tp, sp):
    H, W = c.shape[:2]
    d_c, d_g = dev(c), dev(g)
    d_prev = [dev(a) for a in (pc, pg, pl, pm)] if pc is not None else None
    d_out, d_len, d_mom = blank(W * H * 12), blank(W * H * 4), blank(W * H * 8)
    torch.cuda.synchronize()
    pp = [t.data_ptr() for t in d_prev] if d_prev else [0, 0, 0, 0]
    rt.svgf_accumulate_async(view, d_c.data_ptr(), d_g.data_ptr(), pp[0], pp[1], pp[2], pp[3], W, H,
                             d_out.data_ptr(), d_len.data_ptr(), d_mom.data_ptr(), 0, tp, sp)
    rt.svgf_wait()
    return floats(d_out, H, W, 3), words(d_len, H, W), floats(d_mom, H, W, 2)


def gpu_svgf_filter(rt, c, m, n, g, sp):
    H, W = n.shape
    d_c, d_m, d_n, d_g = dev(c), dev(m), dev(n), dev(g)
    d_out, d_var, d_fb = blank(W * H * 12), blank(W * H * 4), blank(W * H * 12)
    d_rgba = blank(W * H * 4, 0)
    torch.cuda.synchronize()
    rt.svgf_filter_async(d_c.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), d_g.data_ptr(), W, H,
                         d_out.data_ptr(), d_var.data_ptr(), d_fb.data_ptr(), d_rgba.data_ptr(), sp)
    rt.svgf_wait()
    return (floats(d_out, H, W, 3), floats(d_var, H, W), floats(d_fb, H, W, 3),
            d_rgba.cpu().numpy().reshape(H, W, 4))


# ---------------------------------------------------------------------------- salted inputs
def salted_filter_case(seed=1, W=W0, H=H0, moments=True):
    """denoise_ref.synthetic_case with salted colour, position, normal and (moments = True)
    moments, and history lengths 1..6 (0 on the texels that are not filterable); (c, m, n, g)."""
    rng = np.random.default_rng(seed)
    c, g = R.synthetic_case(W, H, seed, color_max=100.0)
    m = S.synthetic_moments(c, seed + 1)
    m[~R.filterable(g)] = 0
    n = rng.integers(1, 7, (H, W)).astype(np.uint32)
    n[~R.filterable(g)] = 0
    fields = dict(colour=c, position=g["position"], normal=g["normal"])
    if moments:
        fields["moments"] = m
    N.salt(fields, rng, SHARE, R.filterable(g))
    return c, m, n, g


def salted_pair(identity, seed=2, W=W0, H=H0):
    rng = np.random.default_rng(seed)
    c, g, pc, pg, pl, view = T.synthetic_case(W, H, seed, identity=identity)
    pm = S.synthetic_moments(pc, seed + 1)
    cur, prev = R.filterable(g), R.filterable(pg)
    N.salt(dict(colour=c, position=g["position"], normal=g["normal"], history=pc,
                position_prev=pg["position"], normal_prev=pg["normal"], moments_prev=pm), rng,
           SHARE, dict(colour=cur, position=cur, normal=cur, history=prev, position_prev=prev,
                       normal_prev=prev, moments_prev=prev))
    return c, g, pc, pg, pl, pm, (None if identity else view)


# ---------------------------------------------------------------------------- 1. kernel parity
@pytest.mark.parametrize("sigma_color", [3.0, float("inf")], ids=["sigma3", "sigma_inf"])
@pytest.mark.parametrize("iterations", [1, 2, 3, 5])
def test_denoise_matches_restatement_on_salted_input(tracers, iterations, sigma_color):
    c, _, _, g = salted_filter_case()
    params = abi.make_denoise_params(iterations=iterations, normal_power_log2=2,
                                     sigma_color=sigma_color, sigma_plane=5.0)
    want = R.denoise_params(c, g, params)
    for rule, rt in enumerate(tracers):
        got, rgba = gpu_denoise(rt, c, g, params)
        N.assert_same(got, want, f"rule {rule}")
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


@pytest.mark.parametrize("identity", [True, False], ids=["identity", "reprojection"])
def test_temporal_accumulate_matches_restatement_on_salted_input(tracers, identity):
    c, g, pc, pg, pl, _, view = salted_pair(identity)
    params = abi.make_temporal_params()
    want, want_len = T.accumulate(c, g, pc, pg, pl, view, params)
    for rule, rt in enumerate(tracers):
        got, got_len, rgba = gpu_temporal(rt, c, g, pc, pg, pl, view, params)
        N.assert_same(got, want, f"rule {rule}")
        assert np.array_equal(got_len, want_len), rule
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


@pytest.mark.parametrize("identity", [True, False], ids=["identity", "reprojection"])
def test_svgf_accumulate_matches_restatement_on_salted_input(tracers, identity):
    c, g, pc, pg, pl, pm, view = salted_pair(identity)
    tp, sp = abi.make_temporal_params(), abi.make_svgf_params()
    want, want_len, want_m = S.accumulate(c, g, pc, pg, pl, pm, view, tp, sp)
    got, got_len, got_m = gpu_svgf_accumulate(tracers[0], c, g, pc, pg, pl, pm, view, tp, sp)
    N.assert_same(got, want, "colour")
    N.assert_same(got_m, want_m, "moments")
    assert np.array_equal(got_len, want_len)


@pytest.mark.parametrize("sigma", [2.0, float("inf")], ids=["sigma2", "sigma_inf"])
@pytest.mark.parametrize("below", [1, 4])
def test_svgf_filter_matches_restatement_on_salted_input(tracers, below, sigma):
    """Five passes: both LDS kernels and the direct one."""
    c, m, n, g = salted_filter_case()
    sp = abi.make_svgf_params(iterations=5, spatial_below=below, sigma_luminance=sigma,
                              normal_power_log2=2, sigma_plane=5.0)
    want, want_var, want_first, _ = S.filter_frame(c, m, n, g, sp)
    for rule, rt in enumerate(tracers):
        out, var, first, rgba = gpu_svgf_filter(rt, c, m, n, g, sp)
        N.assert_same(out, want, f"colour (rule {rule})")
        N.assert_same(var, want_var, f"variance (rule {rule})")
        N.assert_same(first, want_first, f"pass-0 colour (rule {rule})")
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


def test_albedo_steps_match_restatement_on_salted_input(cornell):
    rng = np.random.default_rng(6)
    table = AL.albedo_table(cornell.aligned_materials())
    c, g = AL.synthetic_case(W0, H0, 4, len(table), color_max=100.0)
    N.salt(dict(colour=c, position=g["position"], normal=g["normal"]), rng, SHARE, R.filterable(g))
    want_e = AL.demodulate(c, g, table)
    want_o = AL.remodulate(want_e, g, table)
    H, W = c.shape[:2]
    for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST):
        with rvcp_amd.RayTracer(unorm_rule=rule) as rt:
            rt.upload_scene(cornell)
            d_c, d_g = dev(c), dev(g)
            d_e, d_lin, d_rgba = blank(W * H * 12), blank(W * H * 12), blank(W * H * 4, 0)
            torch.cuda.synchronize()
            rt.demodulate_async(d_c.data_ptr(), d_g.data_ptr(), W, H, d_e.data_ptr())
            rt.albedo_wait()
            N.assert_same(floats(d_e, H, W, 3), want_e, f"irradiance (rule {rule})")
            rt.remodulate_async(d_e.data_ptr(), d_g.data_ptr(), W, H, d_lin.data_ptr(),
                                d_rgba.data_ptr())
            rt.albedo_wait()
            N.assert_same(floats(d_lin, H, W, 3), want_o, f"colour (rule {rule})")
            assert np.array_equal(d_rgba.cpu().numpy().reshape(H, W, 4), R.gamma_rgba(want_o, rule))


def poison_colours(rng, *arrays):
    """+-inf and -0.0 into a dozen texels of each colour array of a case of the TAA / TAAU
    generators (which salt NaN colours themselves)."""
    for a in arrays:
        H, W = a.shape[:2]
        for j, t in enumerate(rng.choice(H * W, size=12, replace=False)):
            y, x = divmod(int(t), W)
            a[y, x, j % 3] = (F(np.inf), F(-np.inf), F(-0.0))[j % 3]


def poison_positions(rng, g):
    """NaN, +inf and -inf into one coordinate of a dozen hit texels of the G-buffer."""
    hit = np.flatnonzero(g["face"].reshape(-1) != R.MISS)
    for j, t in enumerate(rng.choice(hit, size=12, replace=False)):
        y, x = divmod(int(t), g.shape[1])
        g["position"][y, x, j % 3] = (F(np.nan), F(np.inf), F(-np.inf))[j % 3]


def differs(a, b):
    return not N.same(a, b).all()


@pytest.mark.parametrize("mode", ["identity", "reprojection"])
def test_taa_resolve_matches_restatement_on_poisoned_input(tracers, mode):
    params = abi.make_taa_params()
    c, g, pr, pl, cv, pv = TA.synthetic_case(W0, H0, 1, params)
    if mode == "identity":
        cv = pv = None
    rng = np.random.default_rng(7)
    clean = TA.resolve(c, g, pr, pl, cv, pv, params)[0]
    poison_colours(rng, c, pr)
    coloured = TA.resolve(c, g, pr, pl, cv, pv, params)[0]
    poison_positions(rng, g)
    want, want_len = TA.resolve(c, g, pr, pl, cv, pv, params)
    # the poison is not lost on unused texels: each kind moves the restatement's output
    assert differs(coloured, clean) and (mode == "identity" or differs(want, coloured))
    for rule, rt in enumerate(tracers):
        H, W = c.shape[:2]
        d_c, d_g, d_pr, d_pl = dev(c), dev(g), dev(pr), dev(pl)
        d_out, d_len, d_rgba = blank(W * H * 12), blank(W * H * 4), blank(W * H * 4, 0)
        torch.cuda.synchronize()
        rt.taa_resolve_async(cv, pv, d_c.data_ptr(), d_g.data_ptr(), d_pr.data_ptr(),
                             d_pl.data_ptr(), W, H, d_out.data_ptr(), d_len.data_ptr(),
                             d_rgba.data_ptr(), params)
        assert rt.taa_wait() >= 0.0
        N.assert_same(floats(d_out, H, W, 3), want, f"rule {rule}")
        assert np.array_equal(words(d_len, H, W), want_len), rule
        assert np.array_equal(d_rgba.cpu().numpy().reshape(H, W, 4), R.gamma_rgba(want, rule)), rule


@pytest.mark.parametrize("mode", ["identity", "reprojection"])
def test_taa_upsample_matches_restatement_on_poisoned_input(tracers, mode):
    s = 2
    params = abi.make_taau_params()
    c, jv, cv, pv, g, pr, pw = TU.synthetic_case(66, 46, s, 1, params)
    if mode == "identity":
        pv = None
    rng = np.random.default_rng(8)
    clean = TU.upsample(c, s, jv, cv, pv, g, pr, pw, params)[0]
    poison_colours(rng, c, pr)
    coloured = TU.upsample(c, s, jv, cv, pv, g, pr, pw, params)[0]
    poison_positions(rng, g)
    want, want_wt = TU.upsample(c, s, jv, cv, pv, g, pr, pw, params)
    # the poison is not lost on unused texels: each kind moves the restatement's output
    assert differs(coloured, clean) and (mode == "identity" or differs(want, coloured))
    h, w = c.shape[:2]
    H, W = h * s, w * s
    for rule, rt in enumerate(tracers):
        d_c, d_pr, d_pw = dev(c), dev(pr), dev(pw)
        d_g = dev(g) if mode == "reprojection" else None
        d_out, d_wt, d_rgba = blank(W * H * 12), blank(W * H * 4), blank(W * H * 4, 0)
        torch.cuda.synchronize()
        rt.taa_upsample_async(s, jv, cv, pv, d_c.data_ptr(), d_g.data_ptr() if d_g is not None
                              else 0, d_pr.data_ptr(), d_pw.data_ptr(), W, H, d_out.data_ptr(),
                              d_wt.data_ptr(), d_rgba.data_ptr(), params)
        assert rt.taau_wait() >= 0.0
        N.assert_same(floats(d_out, H, W, 3), want, f"rule {rule}")
        N.assert_same(floats(d_wt, H, W), want_wt, f"weights (rule {rule})")
        assert np.array_equal(d_rgba.cpu().numpy().reshape(H, W, 4), R.gamma_rgba(want, rule)), rule


# ---------------------------------------------------------------------------- 2. MISS equivalence
@pytest.mark.parametrize("sigma_color", [3.0, float("inf")], ids=["sigma3", "sigma_inf"])
def test_denoise_treats_a_poisoned_texel_as_miss(tracers, sigma_color):
    """Two launches, no restatement: the poisoned frame against the frame whose poisoned texels
    are MISS texels.  Five passes: both LDS kernels and the direct one."""
    c, _, _, g = salted_filter_case(seed=3)
    mask = N.nonfinite(c, g["position"], g["normal"])
    assert mask.any()
    params = abi.make_denoise_params(iterations=5, normal_power_log2=2, sigma_color=sigma_color,
                                     sigma_plane=5.0)
    got, rgba = gpu_denoise(tracers[0], c, g, params)
    want, want_rgba = gpu_denoise(tracers[0], c, N.as_miss(g, mask), params)
    N.assert_same(got, want, "denoise")
    N.assert_same(got[mask], c[mask], "a poisoned centre passes through")
    assert np.array_equal(rgba, want_rgba)


@pytest.mark.parametrize("below", [1, 4])
def test_svgf_filter_treats_a_poisoned_texel_as_miss(tracers, below):
    """As above for B and C, on a frame as the accumulation hands it over: colour and G-buffer
    salted, and a texel with a bad colour -- not live for the accumulation -- with length 0 and
    zero moments, which B reads as no history at all.  (Liveness is per launch: moments salted on
    their own make a texel that B skips and C uses, which no MISS texel is; the parity test above
    and the chain below cover them.)"""
    c, m, n, g = salted_filter_case(seed=4, moments=False)
    bad = N.nonfinite(c)
    assert (bad & R.filterable(g) & ~N.gbuffer_nonfinite(g)).any()
    m[bad], n[bad] = 0, 0
    mask = bad | N.gbuffer_nonfinite(g)
    sp = abi.make_svgf_params(iterations=5, spatial_below=below, normal_power_log2=2,
                              sigma_plane=5.0)
    got = gpu_svgf_filter(tracers[0], c, m, n, g, sp)
    want = gpu_svgf_filter(tracers[0], c, m, n, N.as_miss(g, mask), sp)
    for a, b, what in zip(got[:3], want[:3], ("colour", "variance", "pass-0 colour")):
        N.assert_same(a, b, what)
    assert np.array_equal(got[3], want[3])
    N.assert_same(got[0][mask], c[mask], "a poisoned centre passes through")
    assert not got[1][mask].any()


@pytest.mark.parametrize("identity", [True, False], ids=["identity", "reprojection"])
def test_svgf_accumulate_then_filter_treats_a_poisoned_texel_as_miss(tracers, identity):
    """The chain the library runs, A then B and C, on a salted pair of frames (current colour and
    G-buffer, history colour, moments and G-buffer), two runs compared: whatever A leaves on a
    texel that was not live for it, B and C see it as they see what A leaves on a MISS texel."""
    c, g, pc, pg, pl, pm, view = salted_pair(identity, seed=5)
    cur = N.nonfinite(c, g["position"], g["normal"])
    prev = N.nonfinite(pc, pg["position"], pg["normal"], pm)
    assert (cur & R.filterable(g)).any() and (prev & R.filterable(pg)).any()
    tp = abi.make_temporal_params()
    sp = abi.make_svgf_params(iterations=5, normal_power_log2=2, sigma_plane=5.0)
    rt, runs = tracers[0], []
    for gg, pgg in ((g, pg), (N.as_miss(g, cur), N.as_miss(pg, prev))):
        a, n, m = gpu_svgf_accumulate(rt, c, gg, pc, pgg, pl, pm, view, tp, sp)
        runs.append((a, m, n) + gpu_svgf_filter(rt, a, m, n, gg, sp))
    names = ("accumulated", "moments", "length", "colour", "variance", "pass-0 colour", "bytes")
    for got, want, what in zip(runs[0], runs[1], names):
        if got.dtype == np.float32:
            N.assert_same(got, want, what)
        else:
            assert np.array_equal(got, want), what
    assert not runs[0][2][cur].any() and not runs[0][4][cur].any()
    assert (runs[0][2] >= 1).any() and (runs[0][2] >= 2).any()       # fresh and continued histories


# ---------------------------------------------------------------------------- 3. containment
BAD_TEXELS = [("colour", "nan"), ("colour", "+inf"), ("normal", "nan"), ("normal", N.ZERO_NORMAL),
              ("position", "+inf")]


@pytest.mark.parametrize("field,kind", BAD_TEXELS)
def test_one_bad_texel_in_a_patch_stays_one_pixel(tracers, field, kind):
    size = 81
    c, g = R.coplanar_patch(size, size)
    if field == "colour":
        c = N.single(c, size // 2, size // 2, kind)
    else:
        g[field] = N.single(g[field], size // 2, size // 2, kind)
    for passes in (2, 5):
        params = abi.make_denoise_params(iterations=passes)
        out, _ = gpu_denoise(tracers[0], c, g, params)
        bad = N.nonfinite(out)
        assert np.array_equal(bad, N.nonfinite(c)), f"{passes} passes: {count(bad)} non-finite"
        N.assert_same(out, R.denoise_params(c, g, params), f"{passes} passes")


@pytest.mark.parametrize("kind", ["nan", "+inf"])
@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "feedback"])
def test_one_bad_sample_does_not_outlive_its_frame_in_the_svgf_loop(tracers, feedback, kind):
    """The stateless loop of six frames with a camera at rest, frame 0 with one bad channel."""
    rt, W, H = tracers[0], 65, 65
    rng = np.random.default_rng(4)
    _, g = R.coplanar_patch(W, H)
    frames = [rng.uniform(0.1, 2.0, (H, W, 3)).astype(F) for _ in range(6)]
    frames[0] = N.single(frames[0], H // 2, W // 2, kind)
    tp, sp = abi.make_temporal_params(), abi.make_svgf_params()
    ref = S.Chain(tp, sp, feedback)
    hist, shown, kept = None, [], []
    for k, c in enumerate(frames):
        pc, pl, pm = hist if hist else (None, None, None)
        a, n, m = gpu_svgf_accumulate(rt, c, g, pc, g if hist else None, pl, pm, None, tp, sp)
        out, var, first, _ = gpu_svgf_filter(rt, a, m, n, g, sp)
        hist = (first if feedback else a, n, m)
        shown.append(count(N.nonfinite(out, var)))
        kept.append(count(N.nonfinite(hist[0], hist[2])))
        want, want_var, want_n = ref.frame(c, g, None)
        N.assert_same(out, want, f"frame {k}")
        N.assert_same(var, want_var, f"frame {k} variance")
        assert np.array_equal(n, want_n), k
    assert shown[0] == 1 and kept[0] == 1, (shown, kept)
    assert shown[1:] == [0] * 5 and kept[1:] == [0] * 5, (shown, kept)


# ---------------------------------------------------------------------------- 4. a real scene
@pytest.fixture(scope="module")
def scene():
    sc, g, frames = N.zero_normal_frames()
    rt = rvcp_amd.RayTracer(spp=N.SCENE_SPP)
    rt.upload_scene(sc)
    yield dict(sc=sc, g=g, frames=frames, rt=rt)
    rt.close()


def test_zero_normal_scene_gbuffer_matches_cpu_scan(scene):
    W = H = N.SCENE_SIZE
    out = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene["rt"].render_gbuffer_async(scene["sc"].push_constant(0.0), W, H, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W)
    want = scene["g"]
    for name in ("face", "material"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("position", "normal"):
        N.assert_same(got[name], want[name], name)
    assert not (got["face"] == len(scene["sc"].mesh.aligned_faces()) - 1).any()   # covers no pixel


def test_zero_normal_scene_through_render_svgf(scene):
    """Four frames with feedback against svgf_ref.Chain fed by the oracle's frames."""
    rt, g, W = scene["rt"], scene["g"], N.SCENE_SIZE
    tp, sp = abi.make_temporal_params(), abi.make_svgf_params()
    ref = S.Chain(tp, sp, feedback=True)
    rt.svgf_reset()
    for k, t in enumerate(N.SCENE_TIMES):
        raw = N.nonfinite(scene["frames"][k])
        assert 1 <= count(raw) <= 0.05 * raw.size, count(raw)
        want, want_var, want_len = ref.frame(scene["frames"][k], g, None)
        rgba, lin, var, hist = rt.render_svgf(W, W, t, tp, sp, True, want_linear=True,
                                              want_variance=True, want_history=True)
        N.assert_same(lin, want, f"frame {k} colour")
        N.assert_same(var, want_var, f"frame {k} variance")
        assert np.array_equal(hist, want_len), k
        assert np.array_equal(rgba, R.gamma_rgba(want)), k
        assert not (N.nonfinite(lin, var) & ~raw).any(), (k, count(N.nonfinite(lin, var)))


def test_zero_normal_scene_through_render_denoised(scene):
    rt, g, W = scene["rt"], scene["g"], N.SCENE_SIZE
    params = abi.make_denoise_params()
    for k, t in enumerate(N.SCENE_TIMES):
        raw = N.nonfinite(scene["frames"][k])
        want = R.denoise_params(scene["frames"][k], g, params)
        rgba, lin = rt.render_denoised(W, W, t, params, want_linear=True)
        N.assert_same(lin, want, f"frame {k}")
        assert np.array_equal(rgba, R.gamma_rgba(want)), k
        assert not (N.nonfinite(lin) & ~raw).any(), (k, count(N.nonfinite(lin)))
