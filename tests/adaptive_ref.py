"""numpy restatement of the plan step of adaptive sampling (rvcp_spp_plan_async, csrc/
rvcp_adaptive.hip): from a frame's variance, the colour it belongs to, its history
lengths and its G-buffer to the next frame's per-pixel sample counts.  Every float operation is one
float32 operation in the kernel's order; both sums are integer sums.  TEST INFRASTRUCTURE ONLY.

    l = lum(c)   r = v / (l l + epsilon)   w = r / n   t = min(w, cap) / cap   q = floor(2^20 t)
    q = 0 where the pixel is not filterable, reads a non-finite float, has v not > 0 or n = 0
    S = sum(q)   B = floor(mean_spp npx)   E = B - spp_min npx
    S > 0:  s = spp_min + min(E q // S, spp_max - spp_min)      S = 0:  s = min(spp_min + E // npx, spp_max)
"""
import numpy as np

import denoise_ref as R

f32 = np.float32
SPP_MAP_MAX = 256
Q_ONE = f32(1048576.0)


def lum(c):
    """(0.2126 r + 0.7152 g) + 0.0722 b, each operation rounded (rvcp_post.h)."""
    c = np.asarray(c, dtype=f32)
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def priorities(var, lin, length, gbuf, weight_cap, epsilon):
    """q per pixel (uint32), kernel A."""
    var = np.ascontiguousarray(var, dtype=f32)
    lin = np.ascontiguousarray(lin, dtype=f32)
    n = np.ones(var.shape, np.uint32) if length is None else np.asarray(length, dtype=np.uint32)
    cap, eps = f32(weight_cap), f32(epsilon)
    asks = (R.filterable(gbuf) & np.isfinite(var) & np.isfinite(lin).all(axis=-1) & (n != 0))
    with np.errstate(all="ignore"):
        asks &= var > 0
        l = lum(lin)
        r = var / (l * l + eps)
        w = r / np.maximum(n, 1).astype(f32)
        t = np.where(w < cap, w, cap) / cap
        q = np.where(asks, t * Q_ONE, f32(0.0))
    return np.where(asks, q, 0).astype(np.uint32)


def budget(mean_spp, spp_min, npx):
    """(B, E): floor((double)mean_spp npx), and what it leaves above spp_min for every pixel."""
    B = int(np.floor(float(f32(mean_spp)) * float(npx)))
    return B, max(B - int(spp_min) * int(npx), 0)


def share(q, spp_min, spp_max, mean_spp):
    """The map (uint32) from the priorities, kernel B; python integers: no overflow to think of."""
    q = np.asarray(q, dtype=np.uint32)
    npx = q.size
    _, E = budget(mean_spp, spp_min, npx)
    S = int(q.astype(np.uint64).sum())
    room = int(spp_max) - int(spp_min)
    if S == 0:
        return np.full(q.shape, min(int(spp_min) + E // npx, int(spp_max)), np.uint32)
    extra = (np.uint64(E) * q.astype(np.uint64)) // np.uint64(S)      # E q < 2^59
    return (np.uint64(spp_min) + np.minimum(extra, np.uint64(room))).astype(np.uint32)


def plan(var, lin, length, gbuf, params):
    """(map [H, W] uint32, planned_samples) of rvcp_spp_plan_async; params: a record of
    abi.ADAPTIVE_PARAMS_DTYPE or a dict of its fields."""
    g = lambda k: params[k]                                             # noqa: E731
    q = priorities(var, lin, length, gbuf, g("weight_cap"), g("epsilon"))
    m = share(q, int(g("spp_min")), int(g("spp_max")), g("mean_spp"))
    return m, int(m.astype(np.uint64).sum())


def uniform_count(params):
    """The count of the uniform map a chain's history starts with."""
    fl = int(np.floor(float(f32(params["mean_spp"]))))
    return min(max(fl, int(params["spp_min"])), int(params["spp_max"]))


def clamp_map(m):
    """What the pre-pass makes of a map's words."""
    return np.clip(np.asarray(m, dtype=np.uint32), 1, SPP_MAP_MAX).astype(np.uint32)


DEFAULTS = dict(spp_min=1, spp_max=32, mean_spp=4.0, weight_cap=0.0625, epsilon=1e-2, _pad=0)
