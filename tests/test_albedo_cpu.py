"""Albedo demodulation, the part that needs no GPU: the exported symbols and
their binding; the numpy restatement (tests/albedo_ref.py) held to every case of the definition,
to a constant irradiance under a checker of materials (which the demodulated filter returns and
the plain filter smears) and to the quality gates on scene.checker_floor_scene()."""
import ctypes
import functools
import re
import subprocess

import numpy as np
import pytest

import albedo_ref as A
import denoise_ref as R
import svgf_ref as S
import temporal_ref as T
import oracle as O
import rvcp_amd
from rvcp_amd import abi
from rvcp_amd import scene as _scene
from conftest import ROOT, scene_arrays

MaterialType, checker_floor_scene, cornell_box = (_scene.MaterialType, _scene.checker_floor_scene,
                                                  _scene.cornell_box)

import os

HEADER = os.path.join(ROOT, "include", "rvcp.h")
f32 = np.float32
NEW_SYMBOLS = ("rvcp_demodulate_async", "rvcp_remodulate_async", "rvcp_albedo_wait",
               "rvcp_set_demodulation", "rvcp_get_demodulation")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- symbols, binding
def test_library_exports_the_new_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW_SYMBOLS if f not in exported]
    header = open(HEADER).read()
    L = abi.load()
    for f in NEW_SYMBOLS:
        assert re.search(r"^int " + f + r"\(rvcp_ctx_t \*ctx", header, re.M), f
        assert f in abi.EXPORTED
        assert getattr(L, f).argtypes is not None, f
        assert getattr(L, f).restype is ctypes.c_int, f
    for name in ("demodulate_async", "remodulate_async", "albedo_wait"):
        assert callable(getattr(rvcp_amd.RayTracer, name))
    assert isinstance(rvcp_amd.RayTracer.demodulation, property)
    # only functions were added: the ABI revision and the version string stay
    assert L.rvcp_abi_version() == abi.ABI_VERSION == 2
    assert L.rvcp_version() == b"rvcp-mi355x 0.3.0 (gfx950, ABI 2)"


def test_new_entry_points_reject_a_null_context():
    L = abi.load()
    p = ctypes.c_void_p(1)
    E = abi.RVCP_E_INVALID
    assert L.rvcp_demodulate_async(None, p, p, 8, 8, p, None) == E
    assert L.rvcp_remodulate_async(None, p, p, 8, 8, p, p, None) == E
    assert L.rvcp_albedo_wait(None, None, None) == E
    assert L.rvcp_set_demodulation(None, 1) == E
    assert L.rvcp_get_demodulation(None, p) == E


def test_run_headless_demodulate_argument():
    """interactive.run_headless: `demodulate` sets the tracer's switch before the loop; without
    it the switch is not touched."""
    from rvcp_amd import interactive

    class Stub:
        def __init__(self):
            self.sets = []

        demodulation = property(lambda self: None, lambda self, v: self.sets.append(v))

        def render(self, *a):
            return np.zeros((4, 4, 4), np.uint8)

        render_denoised = render_svgf = render_temporal = render

    for arg, want in ((None, []), (True, [True]), (False, [False])):
        stub = Stub()
        interactive.run_headless(stub, cornell_box(), 2, 4, 4, fixed_dt=0.0, time_seed=float,
                                 demodulate=arg)
        assert stub.sets == want


def test_checker_floor_scene():
    sc = checker_floor_scene()
    base = cornell_box()
    assert len(sc.mesh.faces) == 62 and len(sc.materials) == len(base.materials) + 2
    assert np.array_equal(sc.luminous_face_ids(), base.luminous_face_ids())
    a, b = (sc.materials[-2].albedo, sc.materials[-1].albedo)
    assert sc.materials[-2].ty == sc.materials[-1].ty == MaterialType.Lambertian
    la, lb = float(S.lum(a)), float(S.lum(b))
    assert abs(la - lb) < 0.01 * la and np.abs(a - b).max() > 0.1       # equal luminance, other hue
    faces, verts = sc.mesh.aligned_faces(), sc.mesh.aligned_vertices()
    floor = faces[faces["material_id"] >= len(base.materials)]
    assert len(floor) == 32 and (np.bincount(floor["material_id"])[-2:] == 16).all()
    pos = verts["position"][floor["vertices"].reshape(-1)]
    assert not pos[:, 1].any()                                          # coplanar: y = 0
    assert pos[:, 0].min() == pos[:, 2].min() == -275 and pos[:, 0].max() == pos[:, 2].max() == 275
    # the quads tile the bottom quad: their areas add up to its area
    v = verts["position"][:, :3].astype(np.float64)
    tri = v[floor["vertices"]]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert abs(area.sum() - 550.0 ** 2) < 1e-6 * 550.0 ** 2
    assert len(checker_floor_scene(n=2).mesh.faces) == 30 + 8
    with pytest.raises(ValueError):
        checker_floor_scene(n=0)


# ---------------------------------------------------------------------------- the definition
def one_row(materials, faces=None):
    """A one-row G-buffer of filterable texels with the given material words."""
    g = np.zeros((1, len(materials)), dtype=R.GBUFFER_DTYPE)
    g["material"] = np.asarray(materials, dtype=np.uint32)
    g["face"] = 3 if faces is None else np.asarray(faces, dtype=np.uint32)
    g["normal"][...] = (0, 0, 1)
    return g


def test_unusable_albedo_channels_give_zero():
    table = np.array([[0.5, 0.0, 2.0], [np.nan, np.inf, -1.0], [-0.0, -np.inf, 0.25]], dtype=f32)
    g = one_row([0, 1, 2, 0])
    c = np.array([[[3.0, 7.0, 5.0], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [np.inf, np.nan, 0.0]]], dtype=f32)
    e = A.demodulate(c, g, table)
    assert np.array_equal(e[0, 0], [6.0, 0.0, 2.5])
    assert not e[0, 1].any() and np.array_equal(e[0, 2], [0.0, 0.0, 24.0])
    assert np.isinf(e[0, 3, 0]) and e[0, 3, 1] == 0 and e[0, 3, 2] == 0       # 0 whatever c holds
    o = A.remodulate(np.full((1, 4, 3), 9.0, dtype=f32), g, table)
    assert np.array_equal(o[0, 0], [4.5, 0.0, 18.0])
    assert not o[0, 1].any() and np.array_equal(o[0, 2], [0.0, 0.0, 2.25])
    # a zero channel stays 0 through the whole chain, whatever the neighbours hold
    c2, g2 = R.coplanar_patch(12, 9)
    g2["material"][:, ::2] = 1
    tab = np.array([[0.5, 0.0, 2.0], [0.25, 0.5, 1.0]], dtype=f32)
    out = A.denoise_chain(c2, g2, tab, abi.make_denoise_params())
    zero = g2["material"] == 0
    assert not out[zero][:, 1].any() and (out[~zero][:, 1] > 0).all()
    assert not A.demodulate(c2, g2, tab)[zero][:, 1].any()


def test_off_pixels_pass_through_bit_for_bit():
    table = np.array([[0.5, 0.25, 2.0], [0.1, 0.2, 0.3]], dtype=f32)
    g = one_row([0, 1 | A.EMISSIVE, 2, 0x7FFFFFFF, 0, 1], faces=[3, 3, 3, 3, A.MISS, 3])
    rng = np.random.default_rng(1)
    c = (rng.random((1, 6, 3)) * 100).astype(f32)
    c[0, 2] = (np.nan, -0.0, np.inf)
    for step in (A.demodulate, A.remodulate):
        out = step(c, g, table)
        assert np.array_equal(bits(out)[0, 1:5], bits(c)[0, 1:5])
        assert not np.array_equal(bits(out)[0, 0], bits(c)[0, 0])
        assert not np.array_equal(bits(out)[0, 5], bits(c)[0, 5])
    assert np.array_equal(A.demodulate(c, g, table)[0, 5], c[0, 5] / table[1])
    assert np.array_equal(A.remodulate(c, g, table)[0, 5], c[0, 5] * table[1])


def test_unit_albedos_make_both_steps_the_identity():
    c, g = A.synthetic_case(37, 11, seed=2, n_materials=5)
    table = np.ones((5, 3), dtype=f32)
    assert np.array_equal(bits(A.demodulate(c, g, table)), bits(c))
    assert np.array_equal(bits(A.remodulate(c, g, table)), bits(c))
    assert np.array_equal(A.remodulate_rgba(c[:2, :5], g[:2, :5], table), R.gamma_rgba(c[:2, :5]))


def test_chains_wrap_the_existing_restatements():
    """With unit albedos the chains are the restatements they wrap, bit for bit."""
    c, g, pc, pg, pl, view = T.synthetic_case(24, 16, seed=9)
    table = np.ones((8, 3), dtype=f32)
    tp, sp, dp = T.params(), S.params(), abi.make_denoise_params()
    assert np.array_equal(bits(A.denoise_chain(c, g, table, dp)), bits(R.denoise_params(c, g, dp)))
    ref, got = S.Chain(tp, sp), A.SvgfChain(table, tp, sp)
    tref = A.TemporalChain(table, tp, dp)
    for frame, gb, v in ((pc, pg, None), (c, g, view)):
        for a, b in zip(got.frame(frame, gb, v), ref.frame(frame, gb, v)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        tref.frame(frame, gb, v)
    a0, n0 = T.accumulate(pc, pg, None, None, None, None, tp)
    a1, n1 = T.accumulate(c, g, a0, pg, n0, view, tp)
    assert np.array_equal(bits(tref.hist[0]), bits(a1)) and np.array_equal(tref.hist[2], n1)


# ---------------------------------------------------------------------------- constant irradiance
def test_constant_irradiance_under_a_checker_of_materials():
    """c = a E with power-of-two albedos: c / a = E exactly, so the demodulated default filter
    averages 25 equal values per pass -- each product and sum rounded once, under 51 half-ulps
    (3e-6) -- and returns c within 1e-5 relative, while the plain filter, which has only
    geometry to go on at its defaults, smears the two albedos into each other."""
    c, g, table = A.checker_patch()
    dp = abi.make_denoise_params()
    assert np.isinf(dp["sigma_color"])
    e = A.demodulate(c, g, table)
    assert np.array_equal(e, np.broadcast_to(np.array([0.75, 1.5, 3.0], dtype=f32), e.shape))
    assert np.array_equal(bits(A.remodulate(e, g, table)), bits(c))
    got = A.denoise_chain(c, g, table, dp).astype(np.float64)
    rel = np.abs(got - c) / c
    print(f"demodulated: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-5
    plain = R.denoise_params(c, g, dp).astype(np.float64)
    moved = (np.abs(plain - c) / c).max()
    print(f"plain: max relative move {moved:.3f}")
    assert moved > 0.10


# ---------------------------------------------------------------------------- quality
@functools.lru_cache(maxsize=None)
def quality_inputs():
    """The checker floor at QUALITY_SIZE^2: CPU G-buffer, the checker mask, the oracle at SPP =
    2048 and at SPP = 4 for the eight time seeds."""
    W = H = A.QUALITY_SIZE
    sc = checker_floor_scene()
    arr = scene_arrays(sc)
    g = R.cpu_gbuffer(sc, W, H)
    n_base = len(cornell_box().materials)
    checker = R.filterable(g) & (g["material"] >= n_base)
    truth = O.render(arr, sc.push_constant(77.0), abi.make_config(spp=2048), W, H)[0]
    noisy = [O.render(arr, sc.push_constant(t), abi.make_config(spp=4), W, H)[0]
             for t in A.QUALITY_SEEDS]
    return g, checker, truth, noisy, A.albedo_table(sc.aligned_materials())


def test_quality_view_holds_enough_material_edges():
    g, checker, _, _, _ = quality_inputs()
    m = g["material"]
    pairs = checker[:, :-1] & checker[:, 1:] & (m[:, :-1] != m[:, 1:])
    print(f"checker pixels {int(checker.sum())}, straddling pairs {int(pairs.sum())}")
    assert int(checker.sum()) >= A.MIN_CHECKER_PIXELS
    assert int(pairs.sum()) >= A.MIN_STRADDLING_PAIRS


def test_quality_gate_plain_filter():
    g, checker, truth, noisy, table = quality_inputs()
    dp = abi.make_denoise_params()
    plain = R.rmse(R.denoise_params(noisy[0], g, dp), truth, checker)
    demod = R.rmse(A.denoise_chain(noisy[0], g, table, dp), truth, checker)
    ratio = demod / plain
    print(f"rmse noisy {R.rmse(noisy[0], truth, checker):.4f} plain {plain:.4f} demodulated "
          f"{demod:.4f} ratio {ratio:.4f} gate {A.QUALITY_GATE:.4f}")
    assert abs(ratio - A.RATIO_MEASURED) < 0.005          # the recorded figure is this one
    assert ratio < 1.0 and ratio <= A.QUALITY_GATE


def test_quality_gate_svgf():
    g, checker, truth, noisy, table = quality_inputs()
    tp, sp = T.params(), S.params()
    off, on = S.Chain(tp, sp), A.SvgfChain(table, tp, sp)
    for c in noisy:
        o_off = off.frame(c, g, None)[0]
        o_on, var, n = on.frame(c, g, None)
    assert np.array_equal(n, 8 * R.filterable(g).astype(np.uint32))
    assert np.isfinite(var).all() and (var >= 0).all()
    r_off, r_on = R.rmse(o_off, truth, checker), R.rmse(o_on, truth, checker)
    ratio = r_on / r_off
    print(f"rmse svgf off {r_off:.4f} on {r_on:.4f} ratio {ratio:.4f} gate {A.SVGF_QUALITY_GATE:.4f}")
    assert abs(ratio - A.SVGF_RATIO_MEASURED) < 0.005
    assert ratio < 1.0 and ratio <= A.SVGF_QUALITY_GATE
