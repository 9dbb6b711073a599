"""The device arithmetic primitives on their own, bit for bit: every small device
function the bit-exactness promise rests on -- sqrt_ieee, rcp_ieee, rcp_scan, rcp_scan_fast,
normalize, divs_y / divs_pos, quot_markstein, sphere_accept, pt_sinf, pt_sinf_rand, rand_of /
rnd, pixel_seed, tri_accept, tri_maybe / tri_maybe_a, hit_shade, shadow_stop, cosine_bounce,
pack_rgb8 -- is run by the test harness (tests/devmath/rvcp_devmath.hip: the product source
included unmodified, one elementwise kernel per primitive, the product's compile flags) over the
named input sets of tests/devmath_ref.py and compared with a CPU reference that shares nothing
with the device code.  Comparison is bit equality of every output float and flag; two NaNs count
as equal whatever their payload; nothing else is excused.  A failure names the primitive, the
count and the first (input bits, got bits, want bits).

The conditions on the input sets (both classes of every guard, both sides of every boundary, the
near-halfway generator, the references themselves) are asserted on the CPU by
tests/test_devmath_cpu.py.

Tried in scratch builds of the harness (one line of the kernel sources changed, the harness
rebuilt, this module run on an MI355X through RVCP_DEVMATH_LIB; the unchanged build passes all
26 tests) -- every change fails at least one test, and the tests that fail name it:

  change                                                   failing tests
  rcp_ieee without its class check                         test_rcp_ieee_exponents_boundaries_specials,
                                                           test_normalize, test_triangle_zero_subnormal_
                                                           denominators_and_degenerate_triangles
  quot_refine's last step as fma(r, y, q)                  test_vector_by_scalar_division[divs_y],
    (a -0 numerator gives +0)                              [divs_pos]
  sqrt_fast_ok widened to x >= 0                           test_sqrt_ieee_exponents_boundaries_specials,
                                                           test_normalize, test_sphere_accept,
                                                           test_cosine_bounce
  rcp_scan takes the IEEE division for a zero denominator  test_rcp_scan_is_ieee_except_nan_for_zero_and_
                                                           nan_denominators
  pt_sinf_rand's add replaced by a shift by 30             test_pt_sinf_rand, test_rand_of,
                                                           test_rnd_streams_across_the_counter_that_stops_
                                                           growing, test_pixel_seed_then_draws
  tri_maybe without its 1 + 2^-20 factor                   test_triangle_edges_vertices_and_time_bounds
    (b = 1 + 2^-20 on the exact lattice: |n| = RN(|den| (1 + 2^-20)) > |den|)
  quot_box's upper bound checks one component only         test_vector_by_scalar_division[divs_y],
                                                           [divs_pos]
"""
import numpy as np
import pytest

import devmath
import devmath_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


def _hex(row):
    return "(" + " ".join(f"{int(w):08x}" for w in np.atleast_1d(row)) + ")"


def _check(op, inputs, got, want, where=None, what=""):
    """Bit equality of got and want ([n] or [n, k]; float32 compared as bits with NaN == NaN)
    on the records `where` selects (all by default)."""
    got, want = np.asarray(got), np.asarray(want)
    ok = R.same_bits(got, want)
    if ok.ndim > 1:
        ok = ok.all(axis=tuple(range(1, ok.ndim)))
    if where is not None:
        ok = ok | ~where
    bad = np.nonzero(~ok)[0]
    if len(bad):
        inp = np.ascontiguousarray(inputs).view(U).reshape(len(ok), -1)
        g = np.ascontiguousarray(got).view(U).reshape(len(ok), -1)
        w = np.ascontiguousarray(want).view(U).reshape(len(ok), -1)
        first = "; ".join(f"in {_hex(inp[i])} got {_hex(g[i])} want {_hex(w[i])}" for i in bad[:4])
        pytest.fail(f"{op}{' ' + what if what else ''}: {len(bad)} of {len(ok)} records differ: {first}")


def _f(words):
    return np.ascontiguousarray(words).view(F)


def _unary(op, x, ref, where=None):
    got = _f(devmath.run(op, x))[:, 0]
    _check(op, x, got, ref(x), where=None if where is None else where(x))
    return got


# ---------------------------------------------------------------------------- roots, reciprocals
def test_sqrt_ieee_every_significand():
    _unary("sqrt", R.exhaustive_sqrt(), R.ref_sqrt)


def test_sqrt_ieee_exponents_boundaries_specials():
    _unary("sqrt", R.unary_general(), R.ref_sqrt)


def test_rcp_ieee_every_significand():
    _unary("rcp_ieee", R.exhaustive_rcp(), R.ref_rcp)


def test_rcp_ieee_exponents_boundaries_specials():
    _unary("rcp_ieee", R.unary_general(), R.ref_rcp)


def test_rcp_scan_every_significand():
    _unary("rcp_scan", R.exhaustive_rcp(), R.ref_rcp_scan)


def test_rcp_scan_is_ieee_except_nan_for_zero_and_nan_denominators():
    x = R.unary_general()
    got = _unary("rcp_scan", x, R.ref_rcp_scan)
    z = (x == 0) | np.isnan(x)
    assert np.all(np.isnan(got[z])), "rcp_scan: a zero or NaN denominator must give NaN"
    _check("rcp_scan", x, got, R.ref_rcp(x), where=~z, what="IEEE everywhere else")


def test_rcp_scan_fast_every_significand():
    _unary("rcp_scan_fast", R.exhaustive_rcp(), R.ref_rcp_scan)


def test_rcp_scan_fast_on_its_domain():
    """IEEE for |den| in [2^-126, 2^126], NaN for +-0; unspecified (and unused) elsewhere."""
    _unary("rcp_scan_fast", R.unary_general(), R.ref_rcp_scan, where=R.rcp_scan_fast_domain)


def test_normalize():
    v = R.normalize_inputs()
    got = _f(devmath.run("normalize", v))
    _check("normalize", v, got, R.ref_normalize(v))


# ------------------------------------------------------------------------------------ quotients
@pytest.mark.parametrize("op", ["divs_y", "divs_pos"])
def test_vector_by_scalar_division(op):
    rec = R.divs_inputs()
    got = _f(devmath.run(op, rec))
    _check(op, rec, got, R.ref_divs(rec))


def test_quot_markstein():
    x, s = R.markstein_inputs()
    rec = np.ascontiguousarray(np.stack([x, s], -1))
    got = _f(devmath.run("markstein", rec))[:, 0]
    want = R.ref_div(x, s)
    inr = R.markstein_range(x, s)
    _check("quot_markstein", rec, got, want, where=inr, what="in its range")
    # outside the numerator's range (s inside): both forms are NaN or lie outside
    # [2^-30, 2^30] in magnitude, so both fail t_min <= t <= t_max
    with np.errstate(invalid="ignore"):
        out = ~inr & (s >= R.p2(-30)) & (s <= R.p2(30))

        def rejected(t):
            a = np.abs(t)
            return np.isnan(t) | (a < R.p2(-30)) | (a > R.p2(30))
    assert np.sum(out) >= 1000
    both = rejected(got) & rejected(want)
    _check("quot_markstein", rec, both, np.ones_like(both), where=out, what="outside its range")


def test_sphere_accept():
    rec = R.sphere_inputs()
    w = devmath.run("sphere", rec)
    ok, t, info = R.ref_sphere(rec)
    fr = R.sphere_fast_range(rec, info)
    acc_f, t_f, acc_s, t_s = w[:, 0], _f(w[:, 1]), w[:, 2], _f(w[:, 3])
    _check("sphere_accept<false>", rec, acc_s, ok.astype(U), what="decision")
    _check("sphere_accept<false>", rec, t_s, t, where=ok, what="t")
    _check("sphere_accept<true>", rec, acc_f, ok.astype(U), where=fr, what="decision")
    _check("sphere_accept<true>", rec, t_f, t, where=fr & ok, what="t")
    _check("sphere_accept<true> vs <false>", rec, acc_f, acc_s, where=fr, what="decision")
    _check("sphere_accept<true> vs <false>", rec, t_f, t_s, where=fr & (acc_s == 1), what="t")


# ------------------------------------------------------------------- sine and the random stream
def test_pt_sinf():
    _unary("sinf", R.sinf_inputs(), R.ref_sinf)


def test_pt_sinf_rand():
    _unary("sinf_rand", R.rand_arg_inputs(), R.ref_sinf)


def test_rand_of():
    _unary("rand_of", R.rand_arg_inputs(), R.ref_rand_of)


def test_rnd_streams_across_the_counter_that_stops_growing():
    rec = R.stream_inputs()
    got = _f(devmath.run("rnd_stream", rec, params=[R.STREAM_DRAWS]))
    _check("rnd", rec, got, R.ref_streams(rec))


def test_pixel_seed_then_draws():
    rec = R.pixel_seed_inputs()
    got = _f(devmath.run("pixel_seed", rec, params=[R.SEED_DRAWS]))
    _check("pixel_seed + rnd", rec, got, R.ref_pixel_seed(rec))


# ------------------------------------------------------------------------------------ triangles
def _tri(pairs, what, with_normals=True):
    rays, tris = pairs
    normals = R.tri_normals(len(rays)) if with_normals else np.tile(
        np.array([0, 1, 0] * 3, F), (len(rays), 1))
    rec = R.tri_records(rays, tris, normals)
    w = devmath.run("tri", rec)
    hit, out = R.ref_tri(rays, tris, normals)
    flags = w[:, 0]
    acc = (flags & 1) != 0
    _check("tri_accept", rec, acc, hit, what=f"{what}: decision")
    _check("tri_accept", rec, _f(w[:, 1]), out[:, 0], where=hit, what=f"{what}: t")
    _check("hit_shade", rec, _f(w[:, 3:6]), out[:, 3:6], where=hit, what=f"{what}: position")
    _check("hit_shade", rec, _f(w[:, 6:9]), out[:, 6:9], where=hit, what=f"{what}: normal")
    dom = R.tri_fast_domain(out)
    _check("tri_accept<FAST>", rec, (flags & 8) != 0, hit, where=dom, what=f"{what}: decision")
    _check("tri_accept<FAST>", rec, _f(w[:, 2]), out[:, 0], where=dom & hit, what=f"{what}: t")
    # the pretest is a theorem: no accepted pair fails either form of it
    for bit, name in ((2, "tri_maybe"), (4, "tri_maybe_a"), (16, "tri_maybe(tri_stage1b)")):
        passed = (flags & bit) != 0
        _check(name, rec, passed | ~acc, np.ones_like(acc), what=f"{what}: accepted but pretest failed")
    # and it is the documented bound on the reference's own den, n1, n2
    first, both = R.pretest_ref(out)
    _check("tri_maybe", rec, (flags & 2) != 0, both, what=f"{what}: vs |n| <= RN(|den| (1 + 2^-20))")
    _check("tri_maybe_a", rec, (flags & 4) != 0, first, what=f"{what}: vs |n1| <= RN(|den| (1 + 2^-20))")
    _check("tri_maybe(tri_stage1b)", rec, (flags & 16) != 0, both, what=what)
    return hit, both


def test_triangle_edges_vertices_and_time_bounds():
    _tri(R.tri_exact_pairs(), "exact edge / vertex / t bounds", with_normals=False)


def test_triangle_zero_subnormal_denominators_and_degenerate_triangles():
    _tri(R.tri_den_pairs(), "den +-0 / subnormal / degenerate")


def test_triangle_fuzz_scales():
    _tri(R.tri_scale_pairs(), "scales 1, 2^22 + 2^38, 2^-20")


def test_triangle_pretest_on_small_triangles():
    hit, both = _tri(R.tri_small_pairs(), "small triangles")
    assert np.mean(~both) >= 0.10 and np.sum(hit) >= 1000


# --------------------------------------------------------- shadow stop, cosine bounce, tone map
def test_shadow_stop_claim():
    rec, d, u = R.shadow_inputs()
    stop = _f(devmath.run("shadow_stop", rec))[:, 0]
    neg = rec[:, 1] < 0
    assert np.all(np.isneginf(stop[neg])), "shadow_stop: t_min < 0 must never stop"
    nonfin = ~np.isfinite(rec[:, 5]) & ~neg
    assert not np.any(np.isfinite(stop[nonfin]) & (stop[nonfin] >= 0)), \
        "shadow_stop: a non-finite dist must never stop"
    for frac in (np.ones_like(u), u):
        viol, live = R.shadow_claim_violations(rec, d, frac, stop)
        assert np.sum(live) >= 10000
        if len(viol):
            i = viol[0]
            pytest.fail(f"shadow_stop: {len(viol)} hits at t <= stop leave |hp - p| > dist - eps; "
                        f"first in {_hex(rec[i].view(U))} stop {_hex(stop[i:i + 1].view(U))}")
    # the stop is not so timid that it never fires: within 2^-10 relative of dist - 2 eps
    ok = np.isfinite(stop) & (stop > 0)
    with np.errstate(all="ignore"):
        slack = (rec[:, 5] - 2 * rec[:, 0] - stop) / (np.max(np.abs(rec[:, 2:5]), axis=-1) + rec[:, 5])
    assert np.sum(ok) >= 10000 and np.all(slack[ok] <= 2.0 ** -15)


def test_cosine_bounce():
    rec = R.cosine_inputs()
    got = _f(devmath.run("cosine_bounce", rec, params=[R.COS_K]))
    _check("cosine_bounce", rec, got, R.ref_cosine(rec))


@pytest.mark.parametrize("rule", [0, 1])
def test_pack_rgb8(rule):
    rec = R.pack_inputs(rule)
    got = devmath.run("pack_rgb8", rec, params=R.gamma_table(rule))[:, 0]
    _check(f"pack_rgb8 (unorm rule {rule})", rec, got, R.ref_pack(rec, rule))
