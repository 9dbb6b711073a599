"""Conditions on the input sets and references of tests/devmath_ref.py, on the CPU (no GPU): the
sets reach both classes of every guard and both sides of every boundary the code names, the
near-halfway generator lands next to rounding boundaries, the pretest's theorem is not tested
on pairs that all pass it, and the numpy float32 references are the exactly rounded results
(rational arithmetic, integer square roots).  Conditions, not measurements."""
import math
from fractions import Fraction

import numpy as np
import pytest

import devmath_ref as R

F = np.float32
MIN_CLASS = 1000


def _both_sides(x, e, r=64):
    """x holds 2^e itself and floats within r ulps below and above it."""
    b = int(R.bits(np.array([R.p2(e)]))[0])
    xb = R.bits(x[np.isfinite(x) & (x > 0)]).astype(np.int64)
    return (np.any(xb == b) and np.any((xb < b) & (xb >= b - r)) and np.any((xb > b) & (xb <= b + r)))


def _classes(name, fast):
    nf, ns = int(np.sum(fast)), int(np.sum(~fast))
    assert nf >= MIN_CLASS and ns >= MIN_CLASS, f"{name}: fast {nf}, fallback {ns}"
    return nf, ns


def test_unary_sets_reach_both_classes_and_both_sides_of_every_boundary():
    x = R.unary_general()
    _classes("sqrt_ieee", R.sqrt_fast(x))
    _classes("rcp_ieee / rcp_scan", R.rcp_result_normal(x))
    _classes("rcp_scan_fast (specified / unspecified)", R.rcp_scan_fast_domain(x))
    with np.errstate(invalid="ignore"):
        _classes("pt_sinf", np.abs(R.sinf_inputs()) < F(1.0e30))
    for e in R.ALL_BOUNDS:
        assert _both_sides(x, e), f"2^{e}"
        assert _both_sides(-x, e), f"-2^{e}"
    assert _both_sides(R.sinf_inputs(), math.log2(float(F(1.0e30))))
    # every exponent field, subnormals (0) and inf / NaN (255) included, in both signs
    assert len(np.unique(R.bits(x) >> np.uint32(23))) == 512
    # rcp_scan's deliberate difference has inputs: zeros and NaNs
    assert np.sum(x == 0) >= 2 and np.sum(np.isnan(x)) >= MIN_CLASS
    assert len(R.exhaustive_sqrt()) == 1 << 24 and len(R.exhaustive_rcp()) == 1 << 24
    assert len(R.patterns()) == 1024 and len(np.unique(R.patterns())) == 1024


def test_quotient_sets_reach_both_classes_and_the_guards():
    rec = R.divs_inputs()
    fast = R.divs_fast(rec)
    _classes("divs_y / divs_pos", fast)
    s = rec[:, 3]
    for e in R.BOUNDS_BOX:
        assert _both_sides(s, e, 8), f"s at 2^{e}"
        for k in range(3):
            assert _both_sides(rec[:, k], e, 8) and _both_sides(-rec[:, k], e, 8), f"v[{k}] at 2^{e}"
    # the whole vector must take the IEEE path: exactly one component outside the box, s inside
    with np.errstate(invalid="ignore"):
        a = np.abs(rec[:, :3])
        comp_out = ~((a == 0) | ((a >= R.p2(-50)) & (a <= R.p2(50))))
        s_in = (s >= R.p2(-50)) & (s <= R.p2(50))
    for k in range(3):
        only_k = comp_out[:, k] & (comp_out.sum(-1) == 1) & s_in
        assert np.sum(only_k) >= MIN_CLASS, k
    # -0 and +0 numerators on the fast path
    z = fast & np.any(rec[:, :3] == 0, axis=-1)
    assert np.sum(z & np.any(R.bits(rec[:, :3]) == 0x80000000, axis=-1)) >= MIN_CLASS
    assert np.sum(z & np.any(R.bits(rec[:, :3]) == 0, axis=-1)) >= MIN_CLASS
    x, sm = R.markstein_inputs()
    _classes("quot_markstein (in range / outside)", R.markstein_range(x, sm))
    for e in (-60, 60):
        assert _both_sides(x, e, 4) and _both_sides(-x, e, 4)
    for e in (-30, 30):
        assert _both_sides(sm, e, 8)
    assert len(R.quot_grid()[0]) == 1 << 22


def test_near_halfway_generator_does_its_job():
    x, s, dist = R.near_halfway()
    q = x.astype(np.float64) / s.astype(np.float64)
    # distance from the float64 quotient to the nearest float32 rounding boundary (a midpoint
    # of two neighbouring floats), relative to the quotient
    q32 = q.astype(F)
    mid_up = (q32.astype(np.float64) + np.nextafter(q32, F(np.inf)).astype(np.float64)) / 2
    mid_dn = (q32.astype(np.float64) + np.nextafter(q32, F(-np.inf)).astype(np.float64)) / 2
    rel = np.minimum(np.abs(q - mid_up), np.abs(q - mid_dn)) / np.abs(q)
    assert np.mean(rel <= 2.0 ** -22) >= 0.90
    # much more than the stated condition asks: the integer construction puts a third of the
    # pairs within 2^-20 ulp of a midpoint (|r| / 2S, |r| <= 5), where a Newton step without
    # the exact remainder fails
    assert np.sum(dist < 2.0 ** -20) >= len(dist) // 4
    assert np.mean(rel <= 2.0 ** -40) >= 0.25
    assert np.all(R.divs_fast(np.stack([x, x, x, s], -1)))       # all inside the guarded box


def _is_rn(exact: Fraction, got: float) -> bool:
    """got (a finite float32 value) is the round-to-nearest-even float32 of `exact`."""
    g = F(got)
    lo, hi = np.nextafter(g, F(-np.inf)), np.nextafter(g, F(np.inf))
    e = abs(exact - Fraction(float(g)))
    for nb in (lo, hi):
        if not np.isfinite(nb):
            continue
        o = abs(exact - Fraction(float(nb)))
        if o < e:
            return False
        if o == e and (int(R.bits(np.array([g]))[0]) & 1):
            return False
    return True


def _sample(rng, n, lo=-60, hi=60):
    m = rng.integers(0, 1 << 23, n).astype(np.uint32)
    pat = R.patterns()
    m[::3] = pat[rng.integers(0, len(pat), len(m[::3]))]
    e = rng.integers(lo + 127, hi + 128, n).astype(np.uint32)
    sg = rng.integers(0, 2, n).astype(np.uint32)
    return R.flt((sg << np.uint32(31)) | (e << np.uint32(23)) | m)


def test_numpy_float32_references_are_exactly_rounded():
    rng = np.random.default_rng(99)
    n = 10000
    x, s = _sample(rng, n), _sample(rng, n)
    hx, hs, _ = R.near_halfway()
    x[: n // 4], s[: n // 4] = hx[: n // 4], hs[: n // 4]
    q = R.ref_div(x, s)
    for a, b, c in zip(x.tolist(), s.tolist(), q.tolist()):
        assert _is_rn(Fraction(a) / Fraction(b), c), (a, b, c)
    r = R.ref_rcp(x)
    for a, c in zip(x.tolist(), r.tolist()):
        assert _is_rn(1 / Fraction(a), c), (a, c)
    # sqrt by integers: x = m 2^e with e even; sqrt(x) = sqrt(m 2^(2k)) 2^(e/2 - k); the floor
    # root of m 2^(2k) with k = 40 carries more than 24 bits, and the remainder decides the tie
    y = np.abs(_sample(rng, n, -100, 100))
    y[:512] = R.exhaustive_sqrt()[:: (1 << 24) // 512][:512]
    rt = R.ref_sqrt(y)
    for a, c in zip(y.tolist(), rt.tolist()):
        fa, fc = Fraction(a), Fraction(c)
        assert fc >= 0
        lo_, hi_ = np.nextafter(F(c), F(0)), np.nextafter(F(c), F(np.inf))
        m_lo = (fc + Fraction(float(lo_))) / 2
        m_hi = (fc + Fraction(float(hi_))) / 2
        # c = RN(sqrt(a))  <=>  m_lo <= sqrt(a) <= m_hi  <=>  m_lo^2 <= a <= m_hi^2 (no float32
        # square root is a midpoint of two floats, so ties do not occur)
        assert m_lo * m_lo < fa < m_hi * m_hi, (a, c)
    assert math.isqrt(1 << 48) == 1 << 24          # (integer square root: the exact case below)
    sq = (np.arange(1, 4097, dtype=np.float64) ** 2).astype(F)
    assert np.array_equal(R.ref_sqrt(sq), np.array([math.isqrt(int(v)) for v in sq], dtype=F))


def test_fma32_is_the_exact_float32_fma():
    rng = np.random.default_rng(7)
    n = 4000
    a, b = _sample(rng, n, -20, 20), _sample(rng, n, -20, 20)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F)      # cancellation
    c[::2] = _sample(rng, n, -40, 40)[::2]
    # products that land exactly on a float32 midpoint plus a tiny addend: the double-rounding case
    a[:200] = F(1.0) + F(2.0 ** -12)
    b[:200] = F(1.0) + F(2.0 ** -12)          # a b = 1 + 2^-11 + 2^-24: a midpoint
    c[:200] = (rng.choice([-1.0, 1.0], 200) * 2.0 ** rng.integers(-80, -30, 200)).astype(F)
    got = R.fma32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        assert _is_rn(Fraction(x) * Fraction(y) + Fraction(z), g), (x, y, z, g)


def test_normalize_and_sphere_sets_reach_both_classes():
    v = R.normalize_inputs()
    with np.errstate(all="ignore"):
        d = R.dot32(v, v)
    _classes("normalize", R.sqrt_fast(d))
    for e in R.BOUNDS_SQRT:
        b = int(R.bits(np.array([R.p2(e)]))[0])
        db = R.bits(d[np.isfinite(d)]).astype(np.int64)
        assert np.any(db < b) and np.any(db >= b) and np.any(np.abs(db - b) <= 256), e
    assert np.sum(np.all(v == 0, axis=-1)) >= 1
    assert np.sum(np.any(v == 0, axis=-1) & ~np.all(v == 0, axis=-1)) >= MIN_CLASS
    assert np.sum(~np.all(np.isfinite(v), axis=-1)) >= MIN_CLASS
    rec = R.sphere_inputs()
    ok, t, info = R.ref_sphere(rec)
    fr = R.sphere_fast_range(rec, info)
    _classes("sphere_accept<true> range", fr)
    _classes("sphere numerators in [2^-60, 2^60]", R.sphere_num_in_guard(info)[fr])
    with np.errstate(invalid="ignore"):
        pos = fr & (info["delta"] >= 0)
    assert np.sum(ok & fr) >= MIN_CLASS and np.sum(~ok & pos) >= MIN_CLASS
    assert np.sum(fr & (info["delta"] == 0)) >= 20               # tangent rays, exactly
    assert np.sum(fr & (info["delta"] < 0)) >= MIN_CLASS
    assert np.sum(fr & (rec[:, 3] <= 0)) >= 100                  # negative and zero radii
    for e in (-60, 60):
        a = np.abs(np.concatenate([info["nplus"][fr], info["nminus"][fr]]))
        a = a[np.isfinite(a)]
        assert np.sum((a < R.p2(e)) & (a > R.p2(e - 2))) >= 100 and \
               np.sum((a > R.p2(e)) & (a < R.p2(e + 2))) >= 100, e
    # roots exactly at t_min and at bt
    assert np.sum(fr & ((info["t0"] == rec[:, 10]) | (info["t1"] == rec[:, 10]))) >= 100
    assert np.sum(fr & ((info["t0"] == rec[:, 11]) | (info["t1"] == rec[:, 11]))) >= 100


def test_triangle_sets_hold_the_edge_cases_and_the_pretest_is_not_vacuous():
    rays, tris = R.tri_exact_pairs()
    hit, out = R.ref_tri(rays, tris, None)
    b1, b2 = out[:, 1], out[:, 2]
    assert np.sum(hit & (b1 == 0)) >= 50 and np.sum(hit & (b2 == 0)) >= 50
    assert np.sum(hit & ((b1 + b2).astype(F) == 1)) >= 50
    assert np.sum(hit & (out[:, 0] == rays[:, 6])) >= 50          # t == t_min
    assert np.sum(hit & (out[:, 0] == rays[:, 7])) >= 50          # t == bt
    assert np.sum(~hit) >= 50
    rays, tris = R.tri_den_pairs()
    hit, out = R.ref_tri(rays, tris, None)
    den = out[:, 9]
    assert np.sum(R.bits(den) == 0) >= 10 and np.sum(R.bits(den) == 0x80000000) >= 10
    assert np.sum((den != 0) & (np.abs(den) < R.p2(-126))) >= 50  # subnormal
    rays, tris = R.tri_scale_pairs()
    hit, out = R.ref_tri(rays, tris, R.tri_normals(len(rays)))
    assert np.sum(hit) >= 10000 and np.sum(~hit) >= 10000
    # the pretest's theorem is checked on pairs of which at least 10 % fail it
    rays, tris = R.tri_small_pairs()
    hit, out = R.ref_tri(rays, tris, None)
    first, both = R.pretest_ref(out)
    assert np.mean(~both) >= 0.10 and np.mean(~first) >= 0.10
    assert np.sum(hit) >= MIN_CLASS
    assert not np.any(hit & ~both)          # the theorem itself, on the reference's own numbers


def test_stream_seed_tonemap_and_shadow_sets():
    st = R.stream_inputs()
    assert np.sum(st[:, 1] == F(16777208.0)) >= MIN_CLASS        # 2^24 - 8: the counter stops
    ref = R.ref_streams(st)
    assert np.all(ref[st[:, 1] == F(16777208.0), -1] == F(16777216.0))
    ps = R.pixel_seed_inputs()
    assert set(np.unique(ps[:, 0]).tolist()) == set(R.SEED_TIMES)
    x = R.rand_arg_inputs()
    assert len(x) >= 1 << 20 and x.min() == 1.0 and x.max() == R.RAND_HI
    for rule in (0, 1):
        rec = R.pack_inputs(rule)
        T = R.gamma_table(rule)
        for k in range(3):
            assert np.all(np.isin(T[1:256], rec[:, k]))
        assert np.any(np.isnan(rec)) and np.any(np.isinf(rec)) and np.any(rec < 0) and np.any(rec > 1)
    rec, d, u = R.shadow_inputs()
    assert np.sum(rec[:, 1] < 0) >= 100 and np.sum(~np.isfinite(rec[:, 5])) >= 10


@pytest.mark.parametrize("bad", ["none", "no_margin"])
def test_shadow_claim_check_can_fail(bad):
    """The float64 claim accepts the documented stop and rejects one without its margins."""
    rec, d, u = R.shadow_inputs()
    eps, p, dist = rec[:, 0], rec[:, 2:5], rec[:, 5]
    with np.errstate(all="ignore"):
        M = ((np.max(np.abs(p), axis=-1) + eps).astype(F) + dist).astype(F)
        marg = (F(2.0 ** -18) * ((M + dist).astype(F) + eps).astype(F)).astype(F)
        stop = ((dist - (F(2.0) * eps).astype(F)).astype(F) - marg).astype(F)
        if bad == "no_margin":
            stop = dist.copy()
    viol, live = R.shadow_claim_violations(rec, d, np.ones_like(u), stop)
    assert np.sum(live) >= 10000
    assert (len(viol) == 0) == (bad == "none")
