"""devmath_ref -- named, deterministic input sets for the device arithmetic primitives
(tests/devmath/rvcp_devmath.hip) and their CPU references (TEST INFRASTRUCTURE ONLY).

The references share nothing with the device code: numpy float32 operations (correctly rounded:
checked against rational arithmetic by tests/test_devmath_cpu.py) for roots, reciprocals and
quotients; the C oracle's array entry points for sin, rand, the tone map and the triangle test;
importance_ref.bounce for the cosine bounce; a float32 restatement of the shader's sphere roots
on an exact float32 fma (`fma32`).  Everything here runs on the CPU; the GPU tests
(tests/test_gpu_devmath.py) feed the same arrays to the harness and compare bits.

Every set is built for where its primitive can go wrong: exhaustive significands, every exponent
crossed with a pattern set, +-64 ulps around each guard and result-class boundary the code names,
subnormals, zeros, infinities and NaN.  `classes(op)` splits a set into the fast and the fallback
class of the op's guard by the reference result or the guard's documented range."""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
U = np.uint32
QNAN = U(0x7FC00000)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def flt(b):
    return np.ascontiguousarray(b, dtype=U).view(F)


def p2(e):
    """2^e as float32 (normal range)."""
    return F(2.0) ** F(e)


def same_bits(got, want):
    """Elementwise: equal bits, or both NaN (whatever the payload)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == F:
        g, w = got.view(U), want.view(U)
        return (g == w) | (np.isnan(got) & np.isnan(want))
    return got == want


# ------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def patterns(count=1024, seed=20260):
    """`count` 23-bit significand patterns: low bits, high bits, their complements, runs of ones
    at every position, and a seeded random fill."""
    pat = set(range(128))
    pat |= {k << 16 for k in range(128)}
    pat |= {0x7FFFFF - k for k in range(128)}
    pat |= {0x7FFFFF ^ (k << 16) for k in range(128)}
    for length in range(1, 24):
        for start in range(0, 24 - length):
            pat.add(((1 << length) - 1) << start)
    rng = np.random.default_rng(seed)
    fixed = sorted(pat)[:count]
    pat = set(fixed)
    while len(pat) < count:
        pat.add(int(rng.integers(0, 1 << 23)))
    return np.array(sorted(pat), dtype=U)


def around(x, r=64, both_signs=True):
    """The floats within r ulps of |x| (and their negatives)."""
    b = int(bits(np.array([abs(x)], F))[0])
    a = np.arange(b - r, b + r + 1, dtype=np.int64).astype(U)
    return flt(np.concatenate([a, a | U(0x80000000)]) if both_signs else a)


def specials():
    return flt(np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                         0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                         0x7F7FFFFF, 0xFF7FFFFF], dtype=U))


@functools.lru_cache(None)
def all_exponents():
    """Every exponent field 0..255 (subnormals, inf and NaN included) x patterns() x both signs."""
    e = (np.arange(256, dtype=U) << U(23))[:, None]
    b = (e | patterns()[None, :]).ravel()
    return flt(np.concatenate([b, b | U(0x80000000)]))


# the boundaries the code names: sqrt_fast_ok, divs_y / normalize, the reciprocal's normal-result
# class, the sphere roots' guards
BOUNDS_SQRT = (-100, 100)
BOUNDS_BOX = (-50, 50)
BOUNDS_RCP = (-126, 126)
BOUNDS_SPHERE = (-30, 30, -60, 60)
ALL_BOUNDS = tuple(sorted(set(BOUNDS_SQRT + BOUNDS_BOX + BOUNDS_RCP + BOUNDS_SPHERE)))


@functools.lru_cache(None)
def unary_general():
    """Exponents x patterns, +-64 ulps around every named boundary, the specials."""
    parts = [all_exponents(), specials()]
    parts += [around(p2(e)) for e in ALL_BOUNDS]
    return np.concatenate(parts)


def exhaustive_sqrt():
    """All 2^24 floats of [1, 4)."""
    return flt(np.arange(0x3F800000, 0x40800000, dtype=np.int64).astype(U))


def exhaustive_rcp():
    """All 2^23 floats of [1, 2), both signs."""
    b = np.arange(0x3F800000, 0x40000000, dtype=np.int64).astype(U)
    return flt(np.concatenate([b, b | U(0x80000000)]))


# ------------------------------------------------------------------------------------------
# references: roots and reciprocals
# ------------------------------------------------------------------------------------------
def ref_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(x.astype(F))


def ref_rcp(x):
    with np.errstate(all="ignore"):
        return (F(1.0) / x.astype(F)).astype(F)


def ref_rcp_scan(x):
    """IEEE, except that a zero or NaN denominator gives NaN (the documented difference)."""
    r = ref_rcp(x)
    r[(x == 0) | np.isnan(x)] = np.nan
    return r


def rcp_result_normal(x):
    """The reciprocal's fast class: the IEEE result is a normal number."""
    r = np.abs(ref_rcp(x))
    return np.isfinite(r) & (r >= p2(-126))


def rcp_scan_fast_domain(x):
    """Where rcp_scan_fast is specified: |den| in [2^-126, 2^126] (IEEE) or +-0 (NaN)."""
    a = np.abs(x)
    return (x == 0) | ((a >= p2(-126)) & (a <= p2(126)))


def sqrt_fast(x):
    with np.errstate(invalid="ignore"):
        return (x >= p2(-100)) & (x <= p2(100))


# ------------------------------------------------------------------------------------------
# float32 fma, exact (round-to-odd in float64, then one rounding to float32)
# ------------------------------------------------------------------------------------------
def fma32(a, b, c):
    a, b, c = (np.asarray(t, dtype=F).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact: 48 bits
        s = p + c
        bp = s - p
        err = (p - (s - bp)) + (c - bp)             # TwoSum: s + err = p + c exactly
        fin = np.isfinite(s) & np.isfinite(err)
        even = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(1)) == 0
        fix = fin & (err != 0) & even
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        s = np.where(fix, other, s)
        return s.astype(F)


def dot32(a, b):
    """The contract's dot: fma(z, z', fma(y, y', x x'))."""
    with np.errstate(all="ignore"):
        return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F)))


# ------------------------------------------------------------------------------------------
# quotients
# ------------------------------------------------------------------------------------------
def _scale_pairs(xs, ss, lo=-50, hi=49):
    """Move unit-range (x, s) pairs to exponents inside [2^lo, 2^hi] by a fixed rule."""
    n = len(xs)
    i = np.arange(n, dtype=np.int64)
    ex = (i * 7919) % (hi - lo + 1) + lo
    es = (i * 104729 + 13) % (hi - lo + 1) + lo
    sgn = np.where((i >> 3) & 1, F(-1.0), F(1.0))
    with np.errstate(all="ignore"):
        return (xs * np.ldexp(F(1.0), ex.astype(np.int32)) * sgn).astype(F), \
               (ss * np.ldexp(F(1.0), es.astype(np.int32))).astype(F)


@functools.lru_cache(None)
def quot_grid(nx=2048, ns=2048):
    """(x, s) over an nx x ns grid of significand patterns in [1, 2), exponents spread over the
    box by _scale_pairs."""
    px = flt(U(0x3F800000) | patterns(nx))
    ps = flt(U(0x3F800000) | patterns(ns, seed=7))
    xs = np.repeat(px, ns)
    ss = np.tile(ps, nx)
    return _scale_pairs(xs, ss)


@functools.lru_cache(None)
def near_halfway(count=1 << 16, seed=5):
    """(x, s) whose quotient lies next to a float32 rounding boundary, built with integers.
    Part 1 (the stated construction): significands S, Q in [2^23, 2^24); X = the 24-bit numbers
    on either side of S (Q + 1/2).  Part 2 (the hard cases): S odd, T = 2 Q + 1 chosen by the
    inverse of S modulo 2^24 so that S T = X 2^24 + r with r in {+-1, +-3, +-5}: X / S is
    Q + 1/2 - r / (2 S) in units of the quotient's ulp, |r / (2 S)| < 2^-21.  Returns
    (x, s, dist) with dist the distance to the boundary in ulps of the quotient (float64)."""
    rng = np.random.default_rng(seed)
    pat = patterns().astype(np.int64)
    S = np.concatenate([pat[rng.integers(0, len(pat), count // 2)],
                        rng.integers(0, 1 << 23, count // 2)]) | (1 << 23)
    Q = np.concatenate([rng.integers(0, 1 << 23, count // 2),
                        pat[rng.integers(0, len(pat), count // 2)]]) | (1 << 23)
    # ---- part 1: S (2Q + 1) / 2 lies in [2^46, 2^48); X keeps 24 bits
    P2 = S * (2 * Q + 1)                                   # = 2 S (Q + 1/2), < 2^50
    sh = np.where(P2 >= (1 << 48), 25, 24)                  # 2 X 2^(sh-1) ~ P2
    Xlo = P2 >> sh
    xs1, ss1, d1 = [], [], []
    for X in (Xlo, Xlo + 1):
        ok = (X >= (1 << 23)) & (X < (1 << 24))
        Xk, Sk, Pk, shk = X[ok], S[ok], P2[ok], sh[ok]
        xs1.append(Xk.astype(F))
        ss1.append(Sk.astype(F))
        # quotient X / S in ulps of Q's scale: X 2^(sh-1) / S vs Q + 1/2
        d1.append(np.abs((Xk << shk) - Pk).astype(np.float64) / (2.0 * Sk))
    # ---- part 2
    S2 = S | 1
    inv = S2.copy()
    for _ in range(5):                                     # Newton: inverse modulo 2^24
        inv = (inv * (2 - S2 * inv)) & ((1 << 24) - 1)
    xs2, ss2, d2 = [], [], []
    for r in (1, -1, 3, -3, 5, -5):
        T = (1 << 24) + ((r * inv) & ((1 << 24) - 1))      # odd, in [2^24, 2^25)
        X = (S2 * T - r) >> 24
        assert np.all(X << 24 == S2 * T - r)
        ok = (X < (1 << 24)) | ((X & 1) == 0)              # representable in 24 bits
        xs2.append(X[ok].astype(F))
        ss2.append(S2[ok].astype(F))
        d2.append(np.full(int(ok.sum()), abs(r)) / (2.0 * S2[ok]))
    xs = np.concatenate(xs1 + xs2)
    ss = np.concatenate(ss1 + ss2)
    dist = np.concatenate(d1 + d2)
    e = np.floor(np.log2(xs.astype(np.float64)))           # to [1, 2): exact power-of-two scaling
    xs = (xs / np.exp2(e)).astype(F)
    ss = (ss / F(1 << 23)).astype(F)
    x, s = _scale_pairs(xs, ss)
    return x, s, dist


@functools.lru_cache(None)
def quot_edges():
    """(x, s) with zero numerators of both signs, s and x at and beyond the guards on both
    sides, inf, NaN and subnormals."""
    xs = np.concatenate([specials(), around(p2(-50), 4), around(p2(50), 4), around(p2(-60), 4),
                         around(p2(60), 4), flt(U(0x3F800000) | patterns()[::16])])
    ss = np.concatenate([specials(), around(p2(-50), 8), around(p2(50), 8), around(p2(-30), 8),
                         around(p2(30), 8), np.array([1.0, 3.0, 0.1, 7e-10, 9e12], F)])
    return np.repeat(xs, len(ss)), np.tile(ss, len(xs))


@functools.lru_cache(None)
def markstein_inputs():
    g = quot_grid()
    h = near_halfway()
    e = quot_edges()
    # the grid again inside the Markstein range proper: |x| in [2^-60, 2^60], s in [2^-30, 2^30]
    i = np.arange(len(g[0]), dtype=np.int64)
    with np.errstate(all="ignore"):
        fx, fs = np.frexp(g[0]), np.frexp(g[1])
        xm = np.ldexp(fx[0], ((i * 31) % 120 - 59).astype(np.int32)).astype(F)
        sm = np.ldexp(fs[0], ((i * 17) % 60 - 29).astype(np.int32)).astype(F)
    # numerators outside [2^-60, 2^60] (every exponent, subnormals and non-finite included)
    # over denominators inside [2^-30, 2^30]: both forms must be rejected roots
    xo = all_exponents()[::61]
    so = np.ldexp(flt(U(0x3F800000) | patterns()[np.arange(len(xo)) % 1024]),
                  (np.arange(len(xo)) % 60 - 30).astype(np.int32)).astype(F)
    return np.concatenate([xm, h[0], e[0], xo]), np.concatenate([sm, h[1], e[1], so])


def markstein_range(x, s):
    a = np.abs(x)
    with np.errstate(invalid="ignore"):
        return (a >= p2(-60)) & (a <= p2(60)) & (s >= p2(-30)) & (s <= p2(30))


def ref_div(x, s):
    with np.errstate(all="ignore"):
        return (x.astype(F) / s.astype(F)).astype(F)


@functools.lru_cache(None)
def divs_inputs():
    """Records (v[3], s) for divs_y / divs_pos: the grid and the near-halfway pairs three
    numerators to a shared s; zero numerators of both signs; mixed vectors with one component
    outside the box; s at and beyond the guard; inf, NaN and subnormals."""
    recs = []
    gx, gs = quot_grid()
    nx = 2048
    X = gx.reshape(nx, -1)                         # [x pattern, s pattern]
    S = gs.reshape(nx, -1)
    # three numerators per record, all divided by the first one's s (kept inside the box)
    for k in range(3):
        sel = np.arange(k, nx - 2, 3)
        recs.append(np.stack([X[sel], X[sel + 1], X[sel + 2], S[sel]], -1).reshape(-1, 4))
    hx, hs, _ = near_halfway()
    m = len(hx) - 2
    recs.append(np.stack([hx[:m], hx[1:m + 1], hx[2:m + 2], hs[:m]], -1))
    recs.append(np.stack([hx[:m], np.zeros(m, F), -np.zeros(m, F), hs[:m]], -1))
    # edges: every (x, s) of quot_edges in each slot beside two in-box numerators
    ex, es = quot_edges()
    a = np.full(len(ex), F(0.75))
    b = np.full(len(ex), F(-3.0e5))
    recs += [np.stack([ex, a, b, es], -1), np.stack([a, ex, b, es], -1), np.stack([a, b, ex, es], -1)]
    # mixed vectors: one component outside the box, s inside (the whole vector goes IEEE)
    out = np.concatenate([around(p2(50), 6), around(p2(-50), 6), flt(bits(all_exponents()[::37]))])
    sg = flt(U(0x3F800000) | patterns(64, seed=3))
    o = np.repeat(out, len(sg))
    s = np.tile(sg, len(out)) * F(3.0)
    s = np.ldexp(s, ((np.arange(len(s)) % 3 - 1) * 48).astype(np.int32)).astype(F)   # 2^-48, 1, 2^48
    xg = np.tile(gx[::4099][:len(sg)], len(out))
    recs += [np.stack([o, xg, -xg, s], -1), np.stack([xg, o, xg, s], -1), np.stack([-xg, xg, o, s], -1)]
    return np.ascontiguousarray(np.concatenate(recs).astype(F))


def box_ok(v):
    """quot_box's documented range: every component zero or with magnitude in [2^-50, 2^50]."""
    a = np.abs(v)
    with np.errstate(invalid="ignore"):
        return np.all((a == 0) | ((a >= p2(-50)) & (a <= p2(50))), axis=-1)


def divs_fast(rec):
    s = rec[:, 3]
    with np.errstate(invalid="ignore"):
        return (s >= p2(-50)) & (s <= p2(50)) & box_ok(rec[:, :3])


def ref_divs(rec):
    return ref_div(rec[:, :3], rec[:, 3:4])


# ------------------------------------------------------------------------------------------
# normalize
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def normalize_inputs(seed=11):
    rng = np.random.default_rng(seed)
    recs = []
    # dot on each side of sqrt_fast_ok: one component around 2^+-50 (dot around 2^+-100)
    for e in (-50, 50):
        a = around(p2(e), 64)
        z = np.zeros_like(a)
        recs += [np.stack([a, z, z], -1), np.stack([z, a, z], -1), np.stack([z, -z, a], -1)]
        r = (rng.uniform(0.3, 0.8, (4096, 3)) * float(p2(e))).astype(F)   # |v|^2 near 2^(2e)
        recs.append(r)
    # every scale, random directions and pattern significands
    for e in range(-75, 76):
        v = rng.uniform(-1, 1, (96, 3)).astype(F) * p2(e)
        recs.append(v.astype(F))
    pv = flt(U(0x3F800000) | patterns())
    recs.append(np.stack([pv, np.roll(pv, 1), -np.roll(pv, 2)], -1))
    # zero components, the zero vector, non-finite vectors, subnormals
    sp = specials()
    g = np.array(np.meshgrid(sp, sp, sp, indexing="ij")).reshape(3, -1).T
    recs.append(g)
    recs.append(np.stack([pv, np.zeros_like(pv), -np.zeros_like(pv)], -1))
    return np.ascontiguousarray(np.concatenate(recs).astype(F))


def ref_normalize(v):
    with np.errstate(all="ignore"):
        r = (F(1.0) / np.sqrt(dot32(v, v))).astype(F)
        return (v * r[:, None]).astype(F)


# ------------------------------------------------------------------------------------------
# sin and the random stream (the C oracle)
# ------------------------------------------------------------------------------------------
def _oracle():
    import oracle
    return oracle


@functools.lru_cache(None)
def k_values():
    """Multiples of pi to test: small k, powers of two and their neighbours, pattern-derived k
    up to 2^23."""
    ks = set(range(0, 2049))
    for e in range(1, 24):
        ks |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    p = patterns().astype(np.int64)
    for sh in (0, 3, 7, 11, 15):
        ks |= set(((p | (1 << 23)) >> (sh + 1)).tolist())
    return np.array(sorted(k for k in ks if 0 <= k <= (1 << 23)), dtype=np.int64)


def near_k_pi(kmax=1 << 23, r=8):
    k = k_values()
    k = k[k <= kmax]
    c = bits((k.astype(np.float64) * np.pi).astype(F)).astype(np.int64)
    b = (c[:, None] + np.arange(-r, r + 1)[None, :]).ravel()
    return flt(b[(b >= 0)].astype(U))


@functools.lru_cache(None)
def sinf_inputs():
    x = near_k_pi()
    return np.concatenate([x, -x, around(F(1.0e30), 64), specials(), unary_general()])


RAND_HI = F(16777220.0)         # 2^24 + 4


@functools.lru_cache(None)
def rand_arg_inputs(seed=17):
    """rand()'s arguments, [1, 2^24 + 4]: a stratified 2^20 subset, the neighbours of every
    k pi in range (the parity flip) and the ends."""
    rng = np.random.default_rng(seed)
    n = 1 << 20
    w = (float(RAND_HI) - 1.0) / n
    x = (1.0 + (np.arange(n) + rng.random(n)) * w).astype(F)
    kp = near_k_pi()
    ends = np.concatenate([around(F(1.0), 8, False), around(RAND_HI, 8, False)])
    x = np.concatenate([x, kp, ends])
    return np.ascontiguousarray(x[(x >= F(1.0)) & (x <= RAND_HI)])


def ref_sinf(x):
    return _oracle().sinf_array(x)


def ref_rand_of(x):
    return _oracle().rand_of_array(x)


STREAM_DRAWS = 32


@functools.lru_cache(None)
def stream_inputs():
    """(seed, idx) stream starts: seeds = fracts from the pattern set, 0 and 1; starts at 0,
    mid-range and 2^24 - 8 (the counter that stops growing)."""
    seeds = np.concatenate([flt(U(0x3F800000) | patterns()) - F(1.0), np.array([0.0, 1.0], F)]).astype(F)
    starts = np.array([0.0, 1000.0, 8388600.0, 16777208.0, 16777215.0, 16777216.0], F)
    return np.ascontiguousarray(np.stack([np.repeat(seeds, len(starts)),
                                          np.tile(starts, len(seeds))], -1))


def ref_streams(rec, draws=STREAM_DRAWS):
    return _oracle().rand_sequence_from(rec[:, 0], rec[:, 1], draws)


SEED_TIMES = (0.0, 1.5, 999.0, 421.25)          # tests/test_gpu_parity.py::test_bitexact_time_seeds
SEED_WIDTHS = (1, 3, 37, 1000, 1024, 4096)
SEED_DRAWS = 8


@functools.lru_cache(None)
def pixel_seed_inputs():
    """(time, u, v): every pixel-centre u of each width against a spread of that width's v."""
    recs = []
    for W in SEED_WIDTHS:
        c = ((np.arange(W, dtype=F) + F(0.5)) / F(W)).astype(F)
        vs = c[np.unique(np.linspace(0, W - 1, 7).astype(int))]
        for t in SEED_TIMES:
            u = np.repeat(c, len(vs))
            v = np.tile(vs, len(c))
            recs.append(np.stack([np.full(len(u), t, F), u, v], -1))
    return np.ascontiguousarray(np.concatenate(recs).astype(F))


def ref_pixel_seed(rec, draws=SEED_DRAWS):
    return _oracle().rand_sequence_array(rec, draws)


# ------------------------------------------------------------------------------------------
# triangles (the C oracle)
# ------------------------------------------------------------------------------------------
def _perm_sign(a, k):
    """Permute the axes of [n, 3] vectors and flip signs by rule k (the same for a whole pair)."""
    perm = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)][k % 6]
    sg = np.array([1 if (k >> (3 + j)) & 1 == 0 else -1 for j in range(3)], F)
    return (a[..., list(perm)] * sg).astype(F)


def _pairs(o, d, tmin, bt, v0, v1, v2):
    n = len(o)
    rays = np.concatenate([o, d, np.reshape(tmin, (n, 1)), np.reshape(bt, (n, 1))], -1).astype(F)
    tris = np.concatenate([v0, v1, v2], -1).astype(F)
    return rays, tris


@functools.lru_cache(None)
def tri_exact_pairs():
    """Dyadic pairs where every product is exact: a right triangle with legs 2^i, 2^j in a
    coordinate plane and a ray along the third axis of length 2^m, aimed at barycentrics on a
    lattice that holds the edges (b1 = 0, b2 = 0, b1 + b2 = 1), the vertices and points one
    step outside; t_min and bt at the hit time and one ulp either side."""
    lat = np.array([0.0, 0.25, 0.5, 0.75, 1.0, -2.0 ** -20, 1.0 + 2.0 ** -20, 2.0 ** -23, 1.0 - 2.0 ** -24])
    B1, B2 = (t.ravel() for t in np.meshgrid(lat, lat, indexing="ij"))
    O, D, TMIN, BT, V0, V1, V2 = ([] for _ in range(7))
    k = 0
    for (i, j, m, h) in ((0, 0, 0, 2.0), (3, -2, 1, 5.0), (-4, 5, -3, 0.375), (10, 10, 4, 96.0)):
        x0, y0 = 3.0 * 2.0 ** i, -5.0 * 2.0 ** j
        px, py = x0 + B1 * 2.0 ** i, y0 + B2 * 2.0 ** j
        n = len(px)
        t = h / 2.0 ** m
        for (dt0, dt1) in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (-3, 3)):
            tmin = np.nextafter(F(t), F(np.inf if dt0 > 0 else -np.inf)) if dt0 else F(t)
            bt = np.nextafter(F(t), F(np.inf if dt1 > 0 else -np.inf)) if dt1 else F(t)
            if dt0 == -3:
                tmin, bt = F(t / 4), F(t * 4)
            o = np.stack([px, py, np.full(n, h)], -1)
            d = np.tile([0.0, 0.0, -2.0 ** m], (n, 1))
            v0 = np.tile([x0, y0, 0.0], (n, 1))
            v1 = v0 + [2.0 ** i, 0.0, 0.0]
            v2 = v0 + [0.0, 2.0 ** j, 0.0]
            for a, L in ((o, O), (d, D), (v0, V0), (v1, V1), (v2, V2)):
                L.append(_perm_sign(a.astype(F), k))
            TMIN.append(np.full(n, tmin, F))
            BT.append(np.full(n, bt, F))
            k += 1
    return _pairs(*(np.concatenate(L) for L in (O, D, TMIN, BT, V0, V1, V2)))


@functools.lru_cache(None)
def tri_den_pairs(seed=23):
    """den = +-0 (rays in the triangle's plane), den subnormal or tiny (2^-120 .. 2^-149) and
    degenerate triangles (a zero edge, parallel edges, one point)."""
    rng = np.random.default_rng(seed)
    O, D, TMIN, BT, V0, V1, V2 = ([] for _ in range(7))
    n = 64
    k = 0
    # rays in the plane z = 0 of the triangle: den = +-0 exactly
    for sgn in (1.0, -1.0):
        o = np.stack([rng.integers(-8, 8, n) / 4.0, rng.integers(-8, 8, n) / 4.0, np.zeros(n)], -1)
        d = np.stack([sgn * rng.integers(1, 5, n) / 4.0, rng.integers(-4, 5, n) / 4.0, sgn * np.zeros(n)], -1)
        v0 = np.tile([0.5, 0.25, 0.0], (n, 1))
        for a, L in ((o, O), (d, D), (v0, V0), (v0 + [1.0, 0, 0], V1), (v0 + [0, 2.0, 0], V2)):
            L.append(_perm_sign(a.astype(F), k))
        TMIN.append(np.full(n, 0.0, F))
        BT.append(np.full(n, 1e6, F))
        k += 1
    # den = 2^(i + j + m) tiny: the exact construction of tri_exact_pairs scaled down
    for tot in range(-149, -118):
        i = j = tot // 3
        m = tot - i - j
        b1 = rng.integers(0, 5, 8) / 4.0
        b2 = rng.integers(0, 5, 8) / 4.0
        o = np.stack([b1 * 2.0 ** i, b2 * 2.0 ** j, np.full(8, 2.0 ** m)], -1)
        d = np.tile([0.0, 0.0, -2.0 ** m], (8, 1))
        v0 = np.zeros((8, 3))
        for a, L in ((o, O), (d, D), (v0, V0), (v0 + [2.0 ** i, 0, 0], V1), (v0 + [0, 2.0 ** j, 0], V2)):
            L.append(_perm_sign(a.astype(F), k))
        TMIN.append(np.full(8, 0.0, F))
        BT.append(np.full(8, 1e6, F))
        k += 1
    # degenerate triangles under random rays
    o = rng.uniform(-2, 2, (4 * n, 3))
    d = rng.uniform(-1, 1, (4 * n, 3))
    v0 = rng.uniform(-1, 1, (4 * n, 3))
    e = rng.uniform(-1, 1, (4 * n, 3))
    kind = np.arange(4 * n) % 4
    v1 = np.where((kind == 0)[:, None], v0, v0 + e)                       # e1 = 0 (kind 0)
    v2 = np.where((kind == 1)[:, None], v0, v0 + e * np.where(kind == 2, 2.0, -0.5)[:, None])
    v1 = np.where((kind == 3)[:, None], v0, v1)                          # one point (kind 3)
    v2 = np.where((kind == 3)[:, None], v0, v2)
    for a, L in ((o, O), (d, D), (v0, V0), (v1, V1), (v2, V2)):
        L.append(a.astype(F))
    TMIN.append(np.full(4 * n, 1e-3, F))
    BT.append(np.full(4 * n, 1e6, F))
    return _pairs(*(np.concatenate(L) for L in (O, D, TMIN, BT, V0, V1, V2)))


def _random_pairs(rng, n, scale, offset, tri_size, aim):
    """Rays from random origins aimed at a point of (aim = 1) or near (aim > 1) a random
    triangle of edge length ~ tri_size * scale inside a box of size scale moved by offset."""
    c = rng.uniform(-1, 1, (n, 3))
    v0 = c + rng.uniform(-1, 1, (n, 3)) * tri_size
    v1 = c + rng.uniform(-1, 1, (n, 3)) * tri_size
    v2 = c + rng.uniform(-1, 1, (n, 3)) * tri_size
    w = rng.dirichlet([1, 1, 1], n)
    tgt = w[:, :1] * v0 + w[:, 1:2] * v1 + w[:, 2:] * v2
    tgt = c + (tgt - c) * aim + (aim > 1) * rng.uniform(-1, 1, (n, 3)) * (aim - 1) * 0.2
    o = rng.uniform(-1, 1, (n, 3))
    d = tgt - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    sc = lambda a: (a * scale + offset).astype(F)
    tmin = np.full(n, 1e-3 * scale if scale < 1 else 1e-3, F)
    bt = np.where(rng.random(n) < 0.5, 1e9 * scale, np.linalg.norm(tgt - o, axis=-1) * scale *
                  rng.choice([0.5, 0.999, 1.001, 2.0], n)).astype(F)
    return _pairs(sc(o), d.astype(F), tmin, bt, sc(v0), sc(v1), sc(v2))


@functools.lru_cache(None)
def tri_scale_pairs(seed=29):
    """Random pairs at the scales of tests/fuzz_scenes.py: unit rooms, rooms of scale 2^22 moved
    out by 2^38, rooms of scale 2^-20."""
    rng = np.random.default_rng(seed)
    parts = [_random_pairs(rng, 20000, 1.0, 0.0, 0.5, 1.0),
             _random_pairs(rng, 20000, 2.0 ** 22, np.array([2.0 ** 38, -2.0 ** 38, 2.0 ** 38]), 0.5, 1.0),
             _random_pairs(rng, 20000, 2.0 ** -20, 0.0, 0.5, 1.0),
             _random_pairs(rng, 10000, 1.0, 0.0, 0.5, 1.5)]
    return tuple(np.concatenate(p) for p in zip(*parts))


@functools.lru_cache(None)
def tri_small_pairs(seed=31):
    """The small-triangle set of the pretest: triangles of 1/20 of the room under rays aimed
    anywhere in it (most pairs fail the pretest), with one in eight aimed at the triangle."""
    rng = np.random.default_rng(seed)
    parts = [_random_pairs(rng, 35000, 1.0, 0.0, 0.05, 12.0),
             _random_pairs(rng, 5000, 1.0, 0.0, 0.05, 1.0)]
    return tuple(np.concatenate(p) for p in zip(*parts))


def tri_normals(n, seed=37):
    """Vertex normals for n pairs: unit-length random ones, with every fourth triple (0, 1, 0)."""
    rng = np.random.default_rng(seed)
    nr = rng.normal(size=(n, 3, 3))
    nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
    nr[::4] = [0.0, 1.0, 0.0]
    return np.ascontiguousarray(nr.reshape(n, 9).astype(F))


def tri_records(rays, tris, normals):
    """The harness records of op TRI: ray, v0, e1 = v1 - v0, e2 = v2 - v0 (float32 subtraction, as
    the scene upload forms the TriRecord), the vertex normals."""
    v0, v1, v2 = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    return np.ascontiguousarray(np.concatenate([rays, v0, (v1 - v0).astype(F), (v2 - v0).astype(F),
                                                normals], -1).astype(F))


def ref_tri(rays, tris, normals):
    return _oracle().intersect_array(rays, tris, normals)


def pretest_ref(out):
    """The pretest from the reference's float32 den, n1, n2 (oracle.intersect_array columns
    9..11): |n1| and |n2| at most RN(|den| (1 + 2^-20)).  Returns (first half, both halves)."""
    den, n1, n2 = out[:, 9], out[:, 10], out[:, 11]
    with np.errstate(all="ignore"):
        m = (np.abs(den) * F(1.0 + 2.0 ** -20)).astype(F)
        a = np.abs(n1) <= m
        return a, a & (np.abs(n2) <= m)


def tri_fast_domain(out):
    """Where tri_accept<FAST> is specified: den +-0 or |den| in [2^-126, 2^126]."""
    return rcp_scan_fast_domain(out[:, 9])


# ------------------------------------------------------------------------------------------
# spheres: a float32 restatement of the shader's roots (ray_tracer.comp:260-321)
# ------------------------------------------------------------------------------------------
def ref_sphere(rec):
    """(accept, t, info) for records (ce[3], radius, o[3], d[3], tmin, bt) under the nearest-hit
    rule (the root must be <= bt); info: two_a, delta and the two numerators."""
    ce, rad, o, d, tmin, bt = rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7:10], rec[:, 10], rec[:, 11]
    with np.errstate(all="ignore"):
        co = (o - ce).astype(F)
        a = dot32(d, d)
        two_a = (F(2.0) * a).astype(F)
        b = (F(2.0) * dot32(d, co)).astype(F)
        c = (dot32(co, co) - (rad * rad).astype(F)).astype(F)
        delta = ((b * b).astype(F) - ((F(4.0) * a).astype(F) * c).astype(F)).astype(F)
        sq = np.sqrt(delta).astype(F)
        nplus = ((-b) + sq).astype(F)
        nminus = ((-b) - sq).astype(F)
        t0 = (nplus / two_a).astype(F)
        t1 = (nminus / two_a).astype(F)
        sw = t0 > t1
        t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
        h0 = (tmin <= t0) & (t0 <= bt)
        h1 = (tmin <= t1) & (t1 <= bt)
        ok = ~(delta < 0) & (h0 | h1)
        t = np.where(h0, t0, t1).astype(F)
    return ok, t, dict(two_a=two_a, delta=delta, nplus=nplus, nminus=nminus, t0=t0, t1=t1)


def sphere_fast_range(rec, info):
    """The caller's condition for sphere_accept<true>."""
    with np.errstate(invalid="ignore"):
        return (info["two_a"] >= p2(-30)) & (info["two_a"] <= p2(30)) & \
               (rec[:, 10] >= p2(-29)) & (rec[:, 11] < p2(29))


def sphere_num_in_guard(info):
    """Both numerators inside the Markstein quotient's range [2^-60, 2^60]."""
    with np.errstate(invalid="ignore"):
        ok = np.ones(len(info["delta"]), bool)
        for k in ("nplus", "nminus"):
            a = np.abs(info[k])
            ok &= (a >= p2(-60)) & (a <= p2(60))
        return ok


@functools.lru_cache(None)
def sphere_inputs(seed=41):
    rng = np.random.default_rng(seed)
    recs = []

    def rec(ce, rad, o, d, tmin, bt):
        n = len(o)
        col = lambda a: np.broadcast_to(np.asarray(a, np.float64), (n,)).reshape(n, 1)
        recs.append(np.concatenate([np.broadcast_to(ce, (n, 3)), col(rad), o, d, col(tmin), col(bt)], -1))

    # tangent rays, exact in dyadic numbers: ray along z at distance px = r (1 + k 2^-23)
    for m in (-3, 0, 2, 7):
        for r in (0.5, 1.0, 3.0, 1024.0):
            k = np.arange(-6, 7)
            px = r * (1.0 + k * 2.0 ** -23)
            n = len(k)
            o = np.stack([px, np.zeros(n), np.full(n, -4.0 * r)], -1)
            d = np.tile([0.0, 0.0, 2.0 ** m], (n, 1))
            rec(np.zeros(3), r, o, d, 2.0 ** -20, 2.0 ** 28)
            rec(np.array([8.0, -2.0, 1.0]), r, o + [8.0, -2.0, 1.0], d, 2.0 ** -20, 2.0 ** 28)
    # random rays at several scales: outside and inside origins, negative and zero radii
    for e in (-8, 0, 6, 12):
        n = 6000
        s = 2.0 ** e
        ce = rng.uniform(-1, 1, (n, 3)) * s
        rad = rng.uniform(0.05, 1.0, n) * s * rng.choice([1.0, 1.0, 1.0, -1.0, 0.0], n, p=[.3, .3, .3, .08, .02])
        inside = rng.random(n) < 0.3
        o = np.where(inside[:, None], ce + rng.uniform(-0.5, 0.5, (n, 3)) * np.abs(rad)[:, None],
                     ce + rng.uniform(-3, 3, (n, 3)) * s)
        tgt = ce + rng.uniform(-1.2, 1.2, (n, 3)) * np.abs(rad)[:, None]
        d = tgt - o
        d /= np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-30)
        d *= rng.choice([2.0 ** -10, 0.5, 1.0, 1.0, 3.0, 2.0 ** 12], n)[:, None]
        rec(ce, rad, o, d, 2.0 ** -29 if e < 0 else 1e-3, 2.0 ** 28)
    base = np.concatenate(recs).astype(F)
    # roots straddling tmin and bt: the reference's roots and their float neighbours as bounds
    sub = base[:: max(1, len(base) // 6000)].copy()
    _, _, info = ref_sphere(sub)
    extra = []
    for root in (info["t0"], info["t1"]):
        good = np.isfinite(root) & (root >= p2(-29)) & (root < p2(28))
        for step in (-1, 0, 1):
            nb = np.nextafter(root, F(np.inf) * F(step)) if step else root
            r1 = sub[good].copy()
            r1[:, 10] = nb[good]                       # tmin at the root
            r2 = sub[good].copy()
            r2[:, 11] = nb[good]                       # bt at the root
            extra += [r1, r2]
    recs = [base] + extra
    # numerators at the 2^+-60 guard: |d|^2 = 2^29 (two_a = 2^30), |co| swept so that
    # b = 2 d.co crosses 2^60; and |d|^2 = 2^-31 with tiny |co| for 2^-60
    n = 3000
    for (dl, lo, hi) in ((2.0 ** 14, 43.0, 46.0), (2.0 ** -16, -47.0, -43.0)):
        mag = 2.0 ** rng.uniform(lo, hi, n)
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        d = np.tile([dl, dl, 0.0], (n, 1))
        o = u * mag[:, None]
        rad = mag * rng.uniform(0.5, 1.5, n)
        recs.append(np.concatenate([np.zeros((n, 3)), rad[:, None], o, d,
                                    np.full((n, 1), 2.0 ** -29), np.full((n, 1), 2.0 ** 28)], -1))
    # two_a outside [2^-30, 2^30] (the IEEE form only) and non-finite rays
    n = 2000
    o = rng.uniform(-3, 3, (n, 3))
    d = rng.uniform(-1, 1, (n, 3)) * rng.choice([2.0 ** -20, 2.0 ** 20, 2.0 ** 70], n)[:, None]
    recs.append(np.concatenate([np.zeros((n, 3)), np.ones((n, 1)), o, d, np.full((n, 1), 1e-3),
                                np.full((n, 1), 1e30)], -1))
    sp = specials()
    m = len(sp)
    z = np.zeros(m)
    recs.append(np.stack([z, z, z, z + 1, sp, z, z - 3, z, z, z + 1, z + 1e-3, z + 1e6], -1))
    recs.append(np.stack([z, z, z, sp, z + 0.1, z, z - 3, z, sp, z + 1, z + 1e-3, z + 1e6], -1))
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.concatenate(recs).astype(F))


# ------------------------------------------------------------------------------------------
# shadow_stop: its claim, in float64
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def shadow_inputs(seed=43):
    """(records (eps, t_min, p[3], dist), unit directions d, fractions u in [0, 1]) over the
    scene scales 2^-20 .. 2^38; some t_min negative, some dist non-finite."""
    rng = np.random.default_rng(seed)
    R, Dn, Us = [], [], []
    for e in (-20, -6, 0, 9, 22, 30, 38):
        n = 4000
        s = 2.0 ** e
        off = rng.choice([0.0, 1.0], n)[:, None] * rng.uniform(-1, 1, (n, 3)) * s * 2.0 ** 10
        p = rng.uniform(-1, 1, (n, 3)) * s + off
        dist = s * rng.uniform(1e-3, 2.0, n)
        eps = np.where(rng.random(n) < 0.5, 1e-3, 1e-3 * s)
        tmin = np.where(rng.random(n) < 0.1, -1e-3, rng.choice([0.0, 1e-3], n))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        R.append(np.concatenate([eps[:, None], tmin[:, None], p, dist[:, None]], -1))
        Dn.append(d)
        Us.append(np.where(rng.random(n) < 0.3, 1.0, rng.random(n)))
    rec = np.concatenate(R).astype(F)
    rec[::997, 5] = np.inf
    rec[1::997, 5] = np.nan
    return np.ascontiguousarray(rec), np.concatenate(Dn).astype(F), np.concatenate(Us)


def shadow_claim_violations(rec, d, u, stop):
    """For t = u stop (t <= stop, t >= 0): with hp = (p + eps d) + t d in float64, the claim
    |hp - p| <= dist - eps -- and the claim as stated without the eps offset of the origin,
    |p + t d - p| <= dist - eps.  Returns the indices that break either."""
    eps, p, dist = rec[:, 0].astype(np.float64), rec[:, 2:5].astype(np.float64), rec[:, 5].astype(np.float64)
    st = stop.astype(np.float64)
    with np.errstate(all="ignore"):
        live = np.isfinite(st) & (st >= 0)
        t = np.where(live, st * u, 0.0)
        d64 = d.astype(np.float64)
        hp = (p + eps[:, None] * d64) + t[:, None] * d64
        far = np.linalg.norm(hp - p, axis=-1)
        plain = np.linalg.norm((p + t[:, None] * d64) - p, axis=-1)
        bad = live & ((far > dist - eps) | (plain > dist - eps))
    return np.nonzero(bad)[0], live


# ------------------------------------------------------------------------------------------
# cosine bounce (importance_ref.bounce)
# ------------------------------------------------------------------------------------------
COS_K = F(F(3.1415926) / F(0.8))


@functools.lru_cache(None)
def cosine_inputs(seed=47):
    """Records (alb_pi[3], n[3], p[3], att[3]): axis and random unit normals; unit-ball samples,
    among them p = -n (the sum cancels: the direction is the normal), near-cancelling, tiny
    (the root's guard falls back) and zero samples."""
    rng = np.random.default_rng(seed)
    n = 1500
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
    ax = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)
    nr[::5] = ax[np.arange(len(nr[::5])) % 6]
    nr = nr.astype(F)
    p = rng.uniform(-1, 1, (n, 3))
    p *= (rng.random(n) ** (1 / 3) / np.maximum(np.linalg.norm(p, axis=-1), 1e-9))[:, None]
    p = p.astype(F)
    kind = np.arange(n) % 10
    p[kind == 0] = -nr[kind == 0]
    p[kind == 1] = (-nr[kind == 1] * F(0.37)).astype(F)
    p[kind == 2] = (-nr[kind == 2] * F(0.5) + (rng.normal(size=(int((kind == 2).sum()), 3)) * 1e-7)).astype(F)
    p[kind == 3] = (p[kind == 3] * F(2.0 ** -60)).astype(F)
    p[7::200] = 0.0
    alb = rng.uniform(0, 1, (n, 3)).astype(F) / F(3.1415926)
    att = rng.uniform(0, 1, (n, 3)).astype(F)
    return np.ascontiguousarray(np.concatenate([alb, nr, p, att], -1).astype(F))


def ref_cosine(rec, cos_k=COS_K):
    import importance_ref
    n = len(rec)
    out = np.zeros((n, 6), F)
    with np.errstate(all="ignore"):
        out[:, 0:3] = (rec[:, 9:12] * (rec[:, 0:3] * F(cos_k)).astype(F)).astype(F)
        for i in range(n):
            nn = tuple(F(c) for c in rec[i, 3:6])
            pp = tuple(F(c) for c in rec[i, 6:9])
            out[i, 3:6] = importance_ref.bounce(nn, pp)
    return out


# ------------------------------------------------------------------------------------------
# tone map
# ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def gamma_table(rule):
    """The 257 thresholds pack_rgb8 searches, from the oracle: T[0] = 0, T[k], T[256] = inf."""
    o = _oracle()
    return np.array([o.gamma_threshold(k, rule) for k in range(256)] + [np.inf], dtype=F)


@functools.lru_cache(None)
def pack_inputs(rule):
    T = gamma_table(rule)[1:256]
    b = bits(T).astype(np.int64)
    near = flt((b[:, None] + np.arange(-2, 3)[None, :]).ravel().astype(U))
    rest = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, -1e-30, 1.5, 2.0, 1e30, np.inf, -np.inf,
                                     np.nan], F), specials(), flt(patterns()[::8]),          # subnormals
                           flt(U(0x3F000000) | patterns()), flt(U(0x3A800000) | patterns()[::4]),
                           around(F(1.0), 4)])
    x = np.concatenate([near, rest]).astype(F)
    return np.ascontiguousarray(np.stack([x, np.roll(x, 411), np.roll(x, 977)], -1))


def ref_pack(rec, rule):
    o = _oracle()
    ch = [o.gamma_u8_array(np.ascontiguousarray(rec[:, k]), rule).astype(U) for k in range(3)]
    return ch[0] | (ch[1] << U(8)) | (ch[2] << U(16)) | U(0xFF000000)
