"""albedo_ref -- numpy float32 restatement of albedo demodulation as DESIGN.md §4.12 defines it:
demodulate, remodulate (linear, and RGBA8 through denoise_ref.gamma_rgba), and the three chains
of the library with the demodulation switch set, wrapped around the existing restatements
(TEST INFRASTRUCTURE ONLY: never imported by the package).

It shares no code with csrc/rvcp_albedo.hip, only the contract: float32, one IEEE division resp.
one product per channel, pixels that are not `on` pass through bit for bit.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import svgf_ref as S
import temporal_ref as T

F = np.float32
MISS, EMISSIVE = D.MISS, D.EMISSIVE


def albedo_table(materials) -> np.ndarray:
    """[n, 3] float32: the albedo of every material record, as uploaded."""
    return np.ascontiguousarray(np.asarray(materials)["albedo"], dtype=F).reshape(-1, 3)


def _on_albedo(g, table):
    """(on [H, W], a [H, W, 3]): the pixels that take part and their material's albedo (1 where
    the pixel is off; an id outside the table is never looked up)."""
    table = np.ascontiguousarray(table, dtype=F).reshape(-1, 3)
    m = g["material"] & np.uint32(~np.uint32(EMISSIVE))
    on = (g["face"] != MISS) & ((g["material"] & np.uint32(EMISSIVE)) == 0) & (m < len(table))
    a = np.ones(g.shape + (3,), dtype=F)
    a[on] = table[m[on]]
    return on, a


def _usable(a):
    with np.errstate(invalid="ignore"):
        return (a > 0) & (a < np.inf)


def demodulate(c, g, table):
    """e = usable(a) ? c / a : 0 on the pixels that are on, c elsewhere."""
    c = np.ascontiguousarray(c, dtype=F)
    on, a = _on_albedo(g, table)
    ok = _usable(a)
    with np.errstate(all="ignore"):
        e = np.where(ok, c / np.where(ok, a, F(1)), F(0)).astype(F)
    return np.ascontiguousarray(np.where(on[..., None], e, c), dtype=F)


def remodulate(e, g, table):
    """o = usable(a) ? e * a : 0 on the pixels that are on, e elsewhere (linear colour)."""
    e = np.ascontiguousarray(e, dtype=F)
    on, a = _on_albedo(g, table)
    ok = _usable(a)
    with np.errstate(all="ignore"):
        o = np.where(ok, e * np.where(ok, a, F(1)), F(0)).astype(F)
    return np.ascontiguousarray(np.where(on[..., None], o, e), dtype=F)


def remodulate_rgba(e, g, table, unorm_rule=0):
    """The fused store: RGBA8 of remodulate() exactly as the render stores a linear colour."""
    return D.gamma_rgba(remodulate(e, g, table), unorm_rule)


# ------------------------------------------------------------------------ the chains
def denoise_chain(c, g, table, params):
    """rvcp_render_denoised with the switch set: the remodulated filtered colour."""
    return remodulate(D.denoise_params(demodulate(c, g, table), g, params), g, table)


class TemporalChain:
    """rvcp_render_temporal with the switch set: the history is irradiance."""

    def __init__(self, table, tp, dp=None):
        self.table, self.tp, self.dp = table, tp, dp
        self.hist = None

    def reset(self):
        self.hist = None

    def frame(self, c, g, view):
        """One frame; `view`: the previous frame's camera, or None when it did not move.
        Returns (displayed colour, history length)."""
        e = demodulate(c, g, self.table)
        if self.hist is None:
            a, n = T.accumulate(e, g, None, None, None, None, self.tp)
        else:
            pc, pg, pl = self.hist
            a, n = T.accumulate(e, g, pc, pg, pl, view, self.tp)
        self.hist = (a, g, n)
        show = a if self.dp is None else D.denoise_params(a, g, self.dp)
        return remodulate(show, g, self.table), n


class SvgfChain:
    """rvcp_render_svgf with the switch set: svgf_ref.Chain on irradiance between the two
    steps; the variance is that of the irradiance's luminance."""

    def __init__(self, table, tp, sp, feedback=False):
        self.table = table
        self.chain = S.Chain(tp, sp, feedback)

    def reset(self):
        self.chain.reset()

    def frame(self, c, g, view):
        """Returns (displayed colour, variance, history length)."""
        out, var, n = self.chain.frame(demodulate(c, g, self.table), g, view)
        return remodulate(out, g, self.table), var, n


# ------------------------------------------------------------------------ synthetic inputs
def synthetic_case(W, H, seed, n_materials, color_max=1.0e4):
    """denoise_ref.synthetic_case with material ids over the whole table and, where the frame
    has room, one pixel each of: a colour of 0, material id n_materials (the first outside the
    table), 0x7FFFFFFF, a miss and an emissive texel."""
    c, g = D.synthetic_case(W, H, seed, color_max)
    rng = np.random.default_rng(seed + 1000)
    em = g["material"] & np.uint32(EMISSIVE)
    g["material"] = rng.integers(0, n_materials, (H, W)).astype(np.uint32) | em
    flat_c, flat_g = c.reshape(-1, 3), g.reshape(-1)
    n = flat_g.size
    if n >= 8:
        flat_c[1] = 0
        flat_g["face"][1], flat_g["material"][1] = 5, 0
        flat_g["face"][2], flat_g["material"][2] = 6, n_materials
        flat_g["face"][3], flat_g["material"][3] = 7, 0x7FFFFFFF
        flat_g["face"][4] = MISS
        flat_g["face"][5], flat_g["material"][5] = 8, EMISSIVE | 1
        flat_c[6] = color_max
        flat_g["face"][6], flat_g["material"][6] = 9, 0
    return c, g


def checker_patch(W=40, H=28, cell=2):
    """denoise_ref.coplanar_patch geometry under a checker of cell x cell pixels of materials 0
    and 1, whose albedos are powers of two, lit by the constant irradiance E: c = a E and c / a
    are exact.  Returns (c, g, table)."""
    _, g = D.coplanar_patch(W, H)
    table = np.array([[0.5, 0.25, 1.0], [1.0, 0.5, 0.25]], dtype=F)
    ys, xs = np.mgrid[0:H, 0:W]
    g["material"] = (((ys // cell) + (xs // cell)) & 1).astype(np.uint32)
    E = np.array([0.75, 1.5, 3.0], dtype=F)
    c = np.ascontiguousarray(table[g["material"]] * E, dtype=F)
    return c, g, table


# ------------------------------------------------------------------------ the quality gates
# scene.checker_floor_scene() at 96^2, SPP = 4, against the oracle at SPP =
# 2048 (time seed 77.0), RMSE over the pixels whose face is a checker quad.  (96^2, not the 64^2
# of the other gates: at 64^2 the view holds 407 checker pixels but only 13 horizontally adjacent
# pairs that straddle two materials; at 96^2 954 and 22, above the 200 and 20 the gate asks for.)
#   plain filter: time seed 5.0; rmse(demodulated default denoise) / rmse(plain default denoise)
#   SVGF: 8 frames (time seeds 5.0 ... 12.0), static camera, the defaults without feedback;
#         rmse(frame 8 with the switch on) / rmse(frame 8 with it off)
# Each gate is the measured value plus a quarter of the distance to 1 (denoise_ref.QUALITY_GATE's
# rule); the tests also assert ratio < 1.
QUALITY_SIZE = 96
MIN_CHECKER_PIXELS, MIN_STRADDLING_PAIRS = 200, 20
RATIO_MEASURED = 0.552          # rmse 0.0539 -> 0.0298 (the noisy frame: 0.0668)
QUALITY_GATE = RATIO_MEASURED + (1.0 - RATIO_MEASURED) / 4.0
SVGF_RATIO_MEASURED = 0.308     # rmse 0.0585 -> 0.0180
SVGF_QUALITY_GATE = SVGF_RATIO_MEASURED + (1.0 - SVGF_RATIO_MEASURED) / 4.0
QUALITY_SEEDS = T.QUALITY_SEEDS
