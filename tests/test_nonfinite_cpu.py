"""The non-finite contract of the post-process restatements, on the CPU: a texel
that is not live -- not filterable, or with a NaN or an infinity in a float the step reads -- is
treated exactly as a MISS texel, so each step's output for a poisoned frame equals, bit for bit,
its output for the frame with those texels' face set to MISS; one bad sample stays one bad pixel
through the denoiser, the SVGF chain and a real scene; and on finite inputs the restatement gives
the bits it gave before the rule."""
import numpy as np
import pytest

import albedo_ref as A
import denoise_ref as D
import nonfinite as N
import svgf_ref as S
import temporal_ref as T

F = np.float32
W0, H0 = 45, 31                     # the salted frames
SHARE = 0.03


def count(mask):
    return int(np.count_nonzero(mask))


# ---------------------------------------------------------------------------- salted inputs
def salted_filter_case(seed=1):
    """denoise_ref.synthetic_case with salted colour, position and normal, a variance and
    moments (salted too) and history lengths 1..6; (c, v, m, n, g, hits)."""
    rng = np.random.default_rng(seed)
    c, g = D.synthetic_case(W0, H0, seed, color_max=100.0)
    m = S.synthetic_moments(c, seed + 1)
    v = (rng.random((H0, W0)) ** 3 * 50.0).astype(F)
    n = rng.integers(1, 7, (H0, W0)).astype(np.uint32)
    pos, nrm = g["position"], g["normal"]
    hits = N.salt(dict(colour=c, position=pos, normal=nrm, variance=v, moments=m), rng, SHARE,
                  D.filterable(g))
    return c, v, m, n, g, hits


def salted_pair(seed=2, identity=False):
    """temporal_ref.synthetic_case with every float field of both frames salted, and salted
    history moments; (c, g, pc, pg, pl, pm, view)."""
    rng = np.random.default_rng(seed)
    c, g, pc, pg, pl, view = T.synthetic_case(W0, H0, seed, identity=identity)
    pm = S.synthetic_moments(pc, seed + 1)
    cur, prev = D.filterable(g), D.filterable(pg)
    N.salt(dict(colour=c, position=g["position"], normal=g["normal"], history=pc,
                position_prev=pg["position"], normal_prev=pg["normal"], moments_prev=pm), rng,
           SHARE, dict(colour=cur, position=cur, normal=cur, history=prev, position_prev=prev,
                       normal_prev=prev, moments_prev=prev))
    return c, g, pc, pg, pl, pm, (None if identity else view)


# ---------------------------------------------------------------------------- 1. MISS equivalence
@pytest.mark.parametrize("sigma_color", [3.0, float("inf")])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_atrous_pass_treats_a_poisoned_texel_as_miss(i, sigma_color):
    c, _, _, _, g, _ = salted_filter_case()
    mask = N.nonfinite(c, g["position"], g["normal"])
    assert mask.any() and count(mask) < 0.15 * mask.size
    got = D.atrous_pass(c, g, i, 2, sigma_color, 5.0)
    N.assert_same(got, D.atrous_pass(c, N.as_miss(g, mask), i, 2, sigma_color, 5.0), "pass")
    N.assert_same(got[mask], c[mask], "a poisoned centre passes through")


@pytest.mark.parametrize("identity", [True, False], ids=["identity", "reprojection"])
def test_temporal_accumulate_treats_a_poisoned_texel_as_miss(identity):
    c, g, pc, pg, pl, _, view = salted_pair(identity=identity)
    cur = N.nonfinite(c, g["position"], g["normal"])
    prev = N.nonfinite(pc, pg["position"], pg["normal"])
    assert cur.any() and prev.any()
    out, n = T.accumulate(c, g, pc, pg, pl, view, T.params())
    want, want_n = T.accumulate(c, N.as_miss(g, cur), pc, N.as_miss(pg, prev), pl, view, T.params())
    N.assert_same(out, want, "colour")
    assert np.array_equal(n, want_n)
    N.assert_same(out[cur], c[cur], "a poisoned centre passes through")
    assert not n[cur].any()


@pytest.mark.parametrize("identity", [True, False], ids=["identity", "reprojection"])
def test_svgf_accumulate_treats_a_poisoned_texel_as_miss(identity):
    c, g, pc, pg, pl, pm, view = salted_pair(identity=identity)
    cur = N.nonfinite(c, g["position"], g["normal"])
    prev = N.nonfinite(pc, pg["position"], pg["normal"], pm)
    tp, sp = T.params(), S.params()
    out, n, m = S.accumulate(c, g, pc, pg, pl, pm, view, tp, sp)
    want = S.accumulate(c, N.as_miss(g, cur), pc, N.as_miss(pg, prev), pl, pm, view, tp, sp)
    N.assert_same(out, want[0], "colour")
    assert np.array_equal(n, want[1])
    N.assert_same(m, want[2], "moments")
    N.assert_same(out[cur], c[cur], "a poisoned centre passes through")
    assert not n[cur].any() and not m[cur].any()


@pytest.mark.parametrize("below", [1, 4])
def test_variance_treats_a_poisoned_texel_as_miss(below):
    _, _, m, n, g, _ = salted_filter_case()
    mask = N.nonfinite(m, g["position"], g["normal"])
    sp = S.params(spatial_below=below, normal_power_log2=2, sigma_plane=5.0)
    got = S.variance(m, n, g, sp)
    N.assert_same(got, S.variance(m, n, N.as_miss(g, mask), sp), "variance")
    assert not got[mask].any()


@pytest.mark.parametrize("with_colour", [False, True])
def test_prefilter_treats_a_poisoned_texel_as_miss(with_colour):
    c, v, _, _, g, _ = salted_filter_case()
    cc = c if with_colour else None
    mask = N.nonfinite(v, g["position"], g["normal"], *([c] if with_colour else []))
    got = S.prefilter(v, g, cc)
    N.assert_same(got, S.prefilter(v, N.as_miss(g, mask), cc), "prefilter")
    assert not got[mask].any()


@pytest.mark.parametrize("sigma", [2.0, float("inf")])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_guided_pass_treats_a_poisoned_texel_as_miss(i, sigma):
    c, v, _, _, g, _ = salted_filter_case()
    mask = N.nonfinite(c, v, g["position"], g["normal"])
    sp = S.params(sigma_luminance=sigma, normal_power_log2=2, sigma_plane=5.0)
    co, vo = S.guided_pass(c, v, g, i, sp)
    want_c, want_v = S.guided_pass(c, v, N.as_miss(g, mask), i, sp)
    N.assert_same(co, want_c, "colour")
    N.assert_same(vo, want_v, "variance")
    N.assert_same(co[mask], c[mask], "a poisoned centre passes through")
    assert not vo[mask].any()


def test_albedo_denoise_chain_inherits_the_rule():
    """Between demodulation and remodulation the filter sees the poisoned texels as MISS texels.
    Every albedo of the table is usable, so a poisoned colour stays poisoned as irradiance.  A
    poisoned texel itself is still demodulated and remodulated where a MISS texel is not (its
    finite channels come out as c / a x a, not c), so it is compared with its own irradiance
    passed through."""
    rng = np.random.default_rng(5)
    table = rng.uniform(0.1, 1.0, (6, 3)).astype(F)
    c, g = A.synthetic_case(W0, H0, 3, len(table), color_max=100.0)
    N.salt(dict(colour=c, position=g["position"], normal=g["normal"]), rng, SHARE, D.filterable(g))
    mask = N.gbuffer_nonfinite(g) | N.nonfinite(c)
    params = np.zeros((), dtype=D_PARAMS)
    params["iterations"], params["normal_power_log2"] = 3, 2
    params["sigma_color"], params["sigma_plane"] = 3.0, 5.0
    got = A.denoise_chain(c, g, table, params)
    want = A.denoise_chain(c, N.as_miss(g, mask), table, params)
    N.assert_same(got[~mask], want[~mask], "chain")
    through = A.remodulate(A.demodulate(c, g, table), g, table)
    N.assert_same(got[mask], through[mask], "a poisoned centre passes its irradiance through")


D_PARAMS = np.dtype([("iterations", "<u4"), ("normal_power_log2", "<u4"),
                     ("sigma_color", "<f4"), ("sigma_plane", "<f4")])


# ---------------------------------------------------------------------------- 2. single texels
PW, PH, PY, PX = 21, 17, 8, 10
ALL_KINDS = list(N.KINDS)


def patch(seed=9):
    """A coplanar patch with a random colour per pixel, moments, a variance and lengths."""
    rng = np.random.default_rng(seed)
    _, g = D.coplanar_patch(PW, PH)
    c = rng.uniform(0.1, 4.0, (PH, PW, 3)).astype(F)
    m = S.synthetic_moments(c, seed)
    v = rng.uniform(0.0, 2.0, (PH, PW)).astype(F)
    return c, v, m, g


def poisoned(field, kind):
    """The patch with one texel of one field overwritten; (c, v, m, g)."""
    c, v, m, g = patch()
    if field == "colour":
        c = N.single(c, PY, PX, kind)
    elif field == "variance":
        v = N.single(v, PY, PX, kind)
    elif field == "moments":
        m = N.single(m, PY, PX, kind)
    else:
        g[field] = N.single(g[field], PY, PX, kind)
    return c, v, m, g


def only_here(mask):
    want = np.zeros_like(mask)
    want[PY, PX] = True
    return not (mask & ~want).any()


def cases(*fields):
    return [(f, k) for f in fields
            for k in ALL_KINDS + ([N.ZERO_NORMAL] if f == "normal" else [])]


@pytest.mark.parametrize("field,kind", cases("colour", "position", "normal"))
def test_single_texel_atrous(field, kind):
    c, _, _, g = poisoned(field, kind)
    mask = N.nonfinite(c, g["position"], g["normal"])
    assert count(mask) == (kind in N.POISON)
    for i in range(3):
        for sigma in (3.0, float("inf")):
            got = D.atrous_pass(c, g, i, 2, sigma, 5.0)
            N.assert_same(got, D.atrous_pass(c, N.as_miss(g, mask), i, 2, sigma, 5.0), (i, sigma))
            assert only_here(N.nonfinite(got)), (i, sigma, count(N.nonfinite(got)))
    # all the passes: whatever the texel holds, no other pixel ever turns non-finite
    out = D.denoise(c, g, 5, 2, 3.0, 5.0)
    assert only_here(N.nonfinite(out)), count(N.nonfinite(out))


@pytest.mark.parametrize("field,kind", cases("colour", "variance", "position", "normal"))
def test_single_texel_guided_pass_and_prefilter(field, kind):
    c, v, _, g = poisoned(field, kind)
    mask = N.nonfinite(c, v, g["position"], g["normal"])
    assert count(mask) == (kind in N.POISON)
    pre = S.prefilter(v, g, c)
    N.assert_same(pre, S.prefilter(v, N.as_miss(g, mask), c), "prefilter")
    assert only_here(N.nonfinite(pre))
    for i in range(3):
        for sigma in (2.0, float("inf")):
            sp = S.params(sigma_luminance=sigma, normal_power_log2=2, sigma_plane=5.0)
            co, vo = S.guided_pass(c, v, g, i, sp)
            want = S.guided_pass(c, v, N.as_miss(g, mask), i, sp)
            N.assert_same(co, want[0], (i, sigma))
            N.assert_same(vo, want[1], (i, sigma))
            assert only_here(N.nonfinite(co)) and only_here(N.nonfinite(vo)), (i, sigma)


@pytest.mark.parametrize("field,kind", cases("moments", "position", "normal"))
def test_single_texel_variance(field, kind):
    _, _, m, g = poisoned(field, kind)
    mask = N.nonfinite(m, g["position"], g["normal"])
    n = np.full((PH, PW), 2, dtype=np.uint32)
    n[:, ::2] = 5
    for below in (1, 4):
        sp = S.params(spatial_below=below, normal_power_log2=2, sigma_plane=5.0)
        got = S.variance(m, n, g, sp)
        N.assert_same(got, S.variance(m, n, N.as_miss(g, mask), sp), below)
        assert only_here(N.nonfinite(got)), (below, count(N.nonfinite(got)))
        assert not got[mask].any()


ACC_FIELDS = ("colour", "position", "normal", "history", "position_prev", "normal_prev")


@pytest.mark.parametrize("svgf,field,kind",
                         [(False, f, k) for f, k in cases(*ACC_FIELDS)] +
                         [(True, f, k) for f, k in cases(*ACC_FIELDS, "moments_prev")])
def test_single_texel_accumulate(field, kind, svgf):
    """The identity mapping on the patch: every pixel but the overwritten one gives the bits of
    the clean run, and a poisoned texel leaves what a MISS texel leaves.  (The plain accumulation
    keeps no moments.)"""
    c, _, pm, g = patch()
    pc, _, _, pg = patch(seed=10)
    pl = np.full((PH, PW), 3, dtype=np.uint32)
    tp, sp = T.params(), S.params()

    def run(c, g, pc, pg, pm):
        if svgf:
            return S.accumulate(c, g, pc, pg, pl, pm, None, tp, sp)
        return T.accumulate(c, g, pc, pg, pl, None, tp)

    clean = run(c, g, pc, pg, pm)
    assert (clean[1] == 4).all()
    if field == "colour":
        c = N.single(c, PY, PX, kind)
    elif field == "history":
        pc = N.single(pc, PY, PX, kind)
    elif field == "moments_prev":
        pm = N.single(pm, PY, PX, kind)
    elif field.endswith("_prev"):
        pg[field[:-5]] = N.single(pg[field[:-5]], PY, PX, kind)
    else:
        g[field] = N.single(g[field], PY, PX, kind)
    cur = N.nonfinite(c, g["position"], g["normal"])
    prev = N.nonfinite(pc, pg["position"], pg["normal"], *([pm] if svgf else []))
    assert count(cur | prev) == (kind in N.POISON)
    got = run(c, g, pc, pg, pm)
    want = run(c, N.as_miss(g, cur), pc, N.as_miss(pg, prev), pm)
    here = np.zeros((PH, PW), dtype=bool)
    here[PY, PX] = True
    for a, b, d in zip(got, want, clean):
        if a.dtype == F:
            N.assert_same(a, b, field)
            N.assert_same(a[~here], d[~here], "another pixel changed")
        else:
            assert np.array_equal(a, b) and np.array_equal(a[~here], d[~here])
    if kind in N.POISON:
        assert got[1][PY, PX] == (0 if cur.any() else 1)
        N.assert_same(got[0][PY, PX], c[PY, PX], "the current colour passes through")


@pytest.mark.parametrize("field,kind", cases("colour", "position", "normal"))
def test_single_texel_albedo_denoise_chain(field, kind):
    """albedo_ref.denoise_chain with one texel overwritten: every other pixel as with that texel
    a MISS texel; the texel itself (demodulated and remodulated where a MISS texel is not) as its
    own irradiance passed through."""
    table = np.random.default_rng(5).uniform(0.1, 1.0, (6, 3)).astype(F)
    c, _, _, g = poisoned(field, kind)
    g["material"] = (np.arange(PW * PH, dtype=np.uint32) % len(table)).reshape(PH, PW)
    mask = N.nonfinite(c, g["position"], g["normal"])
    assert count(mask) == (kind in N.POISON)
    params = np.zeros((), dtype=D_PARAMS)
    params["iterations"], params["normal_power_log2"] = 3, 2
    params["sigma_color"], params["sigma_plane"] = 3.0, 5.0
    got = A.denoise_chain(c, g, table, params)
    N.assert_same(got[~mask], A.denoise_chain(c, N.as_miss(g, mask), table, params)[~mask], "chain")
    through = A.remodulate(A.demodulate(c, g, table), g, table)
    N.assert_same(got[mask], through[mask], "the texel passes its irradiance through")
    assert only_here(N.nonfinite(got)), count(N.nonfinite(got))


# ---------------------------------------------------------------------------- 3. containment
# rvcp_denoise_params_default but the passes: normal_power_log2, sigma_color, sigma_plane
DEFAULTS = (7, float("inf"), 0.1)
BAD_TEXELS = [("colour", "nan"), ("colour", "+inf"), ("normal", "nan"), ("normal", N.ZERO_NORMAL),
              ("position", "+inf")]


def bad_patch(field, kind, size=81):
    c, g = D.coplanar_patch(size, size)
    y = x = size // 2
    if field == "colour":
        c = N.single(c, y, x, kind)
    else:
        g[field] = N.single(g[field], y, x, kind)
    return c, g


@pytest.mark.parametrize("field,kind", BAD_TEXELS)
@pytest.mark.parametrize("passes", [2, 5])
def test_one_bad_texel_in_a_patch_stays_one_pixel(passes, field, kind):
    """Before the rule: 169 (2 passes) and all 6561 (5 passes) non-finite pixels for a bad colour,
    25 and 1681 for a bad normal, a zero normal or a bad position."""
    c, g = bad_patch(field, kind)
    out = D.denoise(c, g, passes, *DEFAULTS)
    bad = N.nonfinite(out)
    assert np.array_equal(bad, N.nonfinite(c)), f"{count(bad)} non-finite pixels"
    clean_c, clean_g = D.coplanar_patch(81, 81)
    ok = ~N.nonfinite(c)
    # a constant colour on one plane: every other pixel keeps it, whatever its neighbour holds
    assert np.abs(out[ok] / clean_c[ok] - 1).max() < 1e-6


def chain_frames(kind, W=65, H=65, n=6):
    rng = np.random.default_rng(4)
    _, g = D.coplanar_patch(W, H)
    frames = [rng.uniform(0.1, 2.0, (H, W, 3)).astype(F) for _ in range(n)]
    frames[0] = N.single(frames[0], H // 2, W // 2, kind)
    return frames, g


@pytest.mark.parametrize("kind", ["nan", "+inf"])
@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "feedback"])
def test_one_bad_sample_does_not_outlive_its_frame_in_the_svgf_chain(feedback, kind):
    """Before the rule: 841 shown pixels non-finite in every later frame without feedback; with
    it 25, 81, 169, 289, 441, 625 history texels and 841 -> 2401 shown pixels by frame 5."""
    frames, g = chain_frames(kind)
    chain = S.Chain(T.params(), S.params(), feedback)
    shown, hist = [], []
    for k, c in enumerate(frames):
        out, var, _ = chain.frame(c, g, None)
        shown.append(count(N.nonfinite(out, var)))
        hist.append(count(N.nonfinite(chain.hist[0], chain.hist[3])))
    assert shown[0] == 1 and hist[0] == 1, (shown, hist)
    assert shown[1:] == [0] * 5 and hist[1:] == [0] * 5, (shown, hist)


def assert_chains_agree(a, b, frames, g_of, what):
    """Two svgf_ref.Chains over the same colours, the second under g_of(k)'s G-buffers: every
    output and every piece of the kept history equal, frame by frame."""
    for k, (c, (ga, gb)) in enumerate(zip(frames, g_of)):
        got, want = a.frame(c, ga, None), b.frame(c, gb, None)
        for x, y, name in zip(got + (a.hist[0], a.hist[3]), want + (b.hist[0], b.hist[3]),
                              ("colour", "variance", "length", "history", "history moments")):
            if x.dtype == F:
                N.assert_same(x, y, f"{what}, frame {k}: {name}")
            else:
                assert np.array_equal(x, y), (what, k, name)


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "feedback"])
def test_svgf_chain_treats_a_poisoned_texel_as_miss(feedback):
    """A, B and C as rvcp_render_svgf chains them: the accumulation leaves length 0 and zero
    moments on a texel with a bad colour, and the variance launch must read that as no history
    (not as a live texel whose zero moments enter its neighbours' 7 x 7 estimates).  One NaN on a
    33 x 33 patch, then salted frames (colour in frames 0 and 2, the G-buffer in all)."""
    tp, sp = T.params(), S.params()
    frames, g = chain_frames("nan", 33, 33, 3)
    bad = [N.nonfinite(c) for c in frames]
    assert count(bad[0]) == 1 and not bad[1].any()
    assert_chains_agree(S.Chain(tp, sp, feedback), S.Chain(tp, sp, feedback), frames,
                        [(g, N.as_miss(g, b)) for b in bad], "one NaN")
    rng = np.random.default_rng(11)
    _, g = D.synthetic_case(W0, H0, 7)
    g["material"] &= np.uint32(D.EMISSIVE)              # one material: histories continue
    g["normal"][...] = (0, 0, 1)
    g["position"][..., 2] = 5
    frames = [rng.uniform(0.1, 2.0, (H0, W0, 3)).astype(F) for _ in range(4)]
    filt = D.filterable(g)
    N.salt(dict(position=g["position"], normal=g["normal"], c0=frames[0], c2=frames[2]), rng,
           SHARE, filt)
    masks = [N.gbuffer_nonfinite(g) | N.nonfinite(c) for c in frames]
    a, b = S.Chain(tp, sp, feedback), S.Chain(tp, sp, feedback)
    assert_chains_agree(a, b, frames, [(g, N.as_miss(g, mk)) for mk in masks], "salted")
    assert (a.hist[2] == 4).any() and (a.hist[2][filt] < 4).any()


def test_zero_normal_scene_bad_samples_stay_where_they_fell():
    """Before the rule: 1647, 2082, 2100, 2100 of the 2304 shown pixels non-finite through the
    SVGF chain with feedback, 949 through the default denoiser alone."""
    _, g, frames = N.zero_normal_frames()
    assert not N.gbuffer_nonfinite(g).any()
    chain = S.Chain(T.params(), S.params(), feedback=True)
    counts = []
    for c in frames:
        raw = N.nonfinite(c)
        assert 1 <= count(raw) <= 0.05 * raw.size, count(raw)
        out, var, _ = chain.frame(c, g, None)
        den = D.denoise(c, g, 2, *DEFAULTS)
        counts.append((count(raw), count(N.nonfinite(out, var)), count(N.nonfinite(den))))
        assert not (N.nonfinite(out, var) & ~raw).any(), counts
        assert not (N.nonfinite(den) & ~raw).any(), counts


# ---------------------------------------------------------------------------- 4. finite inputs
def old_atrous_pass(c, g, i, normal_power_log2, sigma_color, sigma_plane):
    """denoise_ref.atrous_pass as it stood before the live rule and the weight-sum guard."""
    c = np.ascontiguousarray(c, dtype=F)
    H, W = c.shape[:2]
    step = 1 << i
    pos, nrm, filt = g["position"], g["normal"], D.filterable(g)
    use_color = not np.isinf(F(sigma_color))
    s2 = D.color_s2(sigma_color, i) if use_color else None
    sp = F(sigma_plane)
    sw = np.zeros((H, W), dtype=F)
    acc = np.zeros((H, W, 3), dtype=F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                valid = filt[P] & filt[Q]
                dn = D._dot3(nrm[P], nrm[Q])
                wn = np.where(dn > 0, dn, F(0)).astype(F)
                for _ in range(int(normal_power_log2)):
                    wn = wn * wn
                d = D._dot3(nrm[P], pos[Q] - pos[P]) / sp
                wz = F(1) / (F(1) + d * d)
                if use_color:
                    e = c[P] - c[Q]
                    wc = F(1) / (F(1) + D._dot3(e, e) / s2)
                else:
                    wc = F(1)
                h = F(D.KERNEL[dy + 2] * D.KERNEL[dx + 2])
                w = ((h * wn) * wz) * wc
                sw[P] = np.where(valid, sw[P] + w, sw[P])
                acc[P] = np.where(valid[..., None], acc[P] + w[..., None] * c[Q], acc[P])
        out = np.where(filt[..., None], acc / sw[..., None], c)
    return np.ascontiguousarray(out, dtype=F)


@pytest.mark.parametrize("W,H", [(45, 31), (67, 5), (8, 8), (1, 1)])
def test_finite_inputs_keep_every_bit(W, H):
    c, g = D.synthetic_case(W, H, seed=W * 100 + H)
    assert not N.nonfinite(c, g["position"], g["normal"]).any()
    for npl2, sigma_color, sigma_plane in ((5, 1.0, 1.0), (8, float("inf"), 30.0), (0, 300.0, 5.0)):
        a = b = c
        for i in range(5):
            a = D.atrous_pass(a, g, i, npl2, sigma_color, sigma_plane)
            b = old_atrous_pass(b, g, i, npl2, sigma_color, sigma_plane)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, npl2)
