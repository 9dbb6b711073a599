"""Cosine-weighted bounce sampling without a GPU (RVCP_SAMPLING_COSINE): the
C-ABI additions (symbols, bindings, the rejections that need no context -- a bad value on a
live context needs a device and lives in test_gpu_importance), the pure-Python restatement
(tests/importance_ref.py) against its committed fixture and against pyref where the two must
agree, the distribution of its directions, and the scene-specialised module's source and key,
which must tell the two modes apart."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import importance_ref as I
import pyref
import rvcp_amd
from conftest import ROOT
from pyref import F
from rvcp_amd import abi

FIXTURE = os.path.join(ROOT, "tests", "golden", "importance_frames.npz")
NEW_SYMBOLS = ("rvcp_set_sampling", "rvcp_get_sampling")
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("pad", "<f4", 3)])


# ------------------------------------------------------------------------------ the interface
def test_library_exports_the_new_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in NEW_SYMBOLS if f not in exported]
    L = abi.load()
    for f in NEW_SYMBOLS:
        assert f in abi.EXPORTED
        assert getattr(L, f).argtypes is not None, f
        assert getattr(L, f).restype is ctypes.c_int, f
    assert isinstance(rvcp_amd.RayTracer.sampling, property)
    assert (abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rvcp.h")).read()
    assert "#define RVCP_SAMPLING_UNIFORM 0" in header and "#define RVCP_SAMPLING_COSINE 1" in header
    assert L.rvcp_abi_version() == abi.ABI_VERSION == 2                 # the ABI did not move


def test_null_context_and_bad_values_are_rejected():
    L = abi.load()
    out = ctypes.c_int32(-5)
    p = ctypes.cast(ctypes.byref(out), ctypes.c_void_p)
    for value in (abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE, 2, -1, 1 << 30):
        assert L.rvcp_set_sampling(None, value) == abi.RVCP_E_INVALID, value
    assert L.rvcp_get_sampling(None, p) == abi.RVCP_E_INVALID
    assert L.rvcp_get_sampling(None, None) == abi.RVCP_E_INVALID
    assert out.value == -5


# --------------------------------------------------------------------------- the restatement
def _check_case(case):
    d = np.load(FIXTURE)
    sc, kw, W, H = I.case_scene(case)
    cfg = abi.make_config(**kw)
    lin, trav = I.render(sc, cfg, sc.push_constant(I.FIXTURE_TIME), W, H)
    want = d[case + "/linear"]
    assert want.shape == (H, W, 3) and d[case + "/rgba"].shape == (H, W, 4)
    bad = np.argwhere(np.any(lin.view(np.uint32) != want.view(np.uint32), axis=-1))
    assert not len(bad), f"{case}: {len(bad)} pixels differ, first {bad[:3].tolist()}"
    assert np.array_equal(trav, d[case + "/traversals_px"])
    assert int(trav.sum()) == int(d[case + "/traversals"]) > W * H * int(cfg["spp"])
    assert np.isfinite(want).all() and (want > 0).any()


def test_fixture_holds_every_case():
    d = np.load(FIXTURE)
    assert {k.split("/")[0] for k in d.files} == set(I.CASES)
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_restatement_equals_fixture():
    _check_case("fuzz2_12x10")


@pytest.mark.slow
@pytest.mark.parametrize("case", [c for c in I.CASES if c != "fuzz2_12x10"])
def test_restatement_equals_fixture_slow(case):
    _check_case(case)


def test_one_bounce_equals_pyref(cornell):
    """With max_bounces = 1 the continuation's direction and weight are never used (the loop
    ends before the next scan), and its rand() calls are the uniform bounce's: the two
    restatements agree bit for bit, traversals included."""
    cfg = abi.make_config(spp=2, max_bounces=1)
    ps = pyref.Scene(cornell.aligned_materials(), cornell.mesh.aligned_vertices(),
                     cornell.mesh.aligned_faces(), cornell.luminous_face_ids())
    P = pyref.params(cfg)
    push = cornell.push_constant(9.0)
    rng = np.random.default_rng(3)
    lit = 0
    for x, y in zip(rng.integers(0, 16, 24).tolist(), rng.integers(0, 16, 24).tolist()):
        a, na = I.render_pixel(ps, P, push, 16, 16, x, y)
        b, nb = pyref.render_pixel(ps, P, push, 16, 16, x, y)
        assert np.array_equal(np.array(a, np.float32).view(np.uint32),
                              np.array(b, np.float32).view(np.uint32)), (x, y)
        assert na == nb
        lit += any(c > 0 for c in a)
    assert lit >= 12
    # ... and with two bounces they part
    cfg2 = abi.make_config(spp=2, max_bounces=2)
    P2 = pyref.params(cfg2)
    differ = sum(I.render_pixel(ps, P2, push, 16, 16, x, 12)[0] != pyref.render_pixel(ps, P2, push, 16, 16, x, 12)[0]
                 for x in range(4, 12))
    assert differ >= 4


@pytest.mark.parametrize("n", [(0.0, 1.0, 0.0), (1.0, 2.0, 3.0)])
def test_direction_statistics(n):
    """64 Rng streams x 300 directions: for a density cos / pi the mean of dot(n, wi) is 2/3
    (uniform sampling gives 1/2), with a standard error of sqrt(1/18 / 19200) = 0.0017; the
    bound 0.02 is twelve of them.  No direction leaves the hemisphere, and every one is a unit
    vector to rounding.  Measured: 0.6665 for n = (0, 1, 0), 0.6690 for normalize((1, 2, 3))."""
    nn = pyref.normalize(pyref.v(*n))
    cos = []
    for s in range(64):
        g = pyref.Rng(F(1.0 + s), F((s % 8 + 0.5) / 8), F((s // 8 + 0.5) / 8))
        for _ in range(300):
            wi = I.bounce(nn, pyref.unit_sphere(g))
            cos.append(float(pyref.dot(nn, wi)))
            assert abs(float(pyref.dot(wi, wi)) - 1.0) < 1e-5
    cos = np.array(cos)
    print(f"n = {n}: mean cos {cos.mean():.4f}, min {cos.min():.3g}")
    assert abs(cos.mean() - 2.0 / 3.0) <= 0.02
    assert cos.min() >= 0.0


def test_direction_falls_back_to_the_normal():
    n = pyref.v(0, 1, 0)
    assert I.bounce(n, pyref.v(0, -0.5, 0)) == n            # n + normalize(p) = 0 exactly
    up = I.bounce(n, pyref.v(0, 0.25, 0))
    assert up == n                                          # normalize(2 n)
    side = I.bounce(n, pyref.v(0.5, 0, 0))                  # normalize(n + x): 45 degrees
    assert abs(float(side[0]) - 2 ** -0.5) < 1e-6 and abs(float(side[1]) - 2 ** -0.5) < 1e-6


# ------------------------------------------------------------------ the specialised modules
def _cornell_records(cornell):
    v = cornell.mesh.aligned_vertices()["position"][:, :3]
    p = v[cornell.mesh.aligned_faces()["vertices"]].astype(np.float32)
    rec = np.zeros(len(p), dtype=TRI_DTYPE)
    rec["v0"] = p[:, 0]
    rec["e1"] = (p[:, 1] - p[:, 0]).astype(np.float32)
    rec["e2"] = (p[:, 2] - p[:, 0]).astype(np.float32)
    return rec


def _module_source(rec, mode):
    fn = abi.load().rvcp_internal_jit_module_source
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    n = fn(rec.ctypes.data, len(rec), mode, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    fn(rec.ctypes.data, len(rec), mode, buf, n + 1)
    return buf.value.decode()


def test_module_source_and_key_differ_between_the_modes(cornell):
    rec = _cornell_records(cornell)
    key = abi.load().rvcp_internal_jit_module_key_for
    key.restype = ctypes.c_uint64
    key.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
    su, sc_ = _module_source(rec, abi.SAMPLING_UNIFORM), _module_source(rec, abi.SAMPLING_COSINE)
    assert su and sc_.startswith(su) and sc_ != su          # the same scan, tagged with the mode
    assert "sampling" in sc_[len(su):] and "sampling" not in su
    ku, kc = key(rec.ctypes.data, len(rec), 0), key(rec.ctypes.data, len(rec), 1)
    assert ku and kc and ku != kc
    assert key(rec.ctypes.data, len(rec), 0) == ku          # ... and a function of the input


def test_cosine_module_compiles_for_gfx950(cornell):
    """hipRTC builds the Cornell box's module with -DRVCP_SAMPLING=1 here, without a GPU; the
    code object is not the default mode's."""
    rec = _cornell_records(cornell)
    fn = abi.load().rvcp_internal_jit_compile_check_sampling
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t),
                   ctypes.c_char_p, ctypes.c_size_t]
    sizes = []
    for mode in (abi.SAMPLING_UNIFORM, abi.SAMPLING_COSINE):
        n = ctypes.c_size_t(0)
        err = ctypes.create_string_buffer(4096)
        rc = fn(rec.ctypes.data, len(rec), mode, ctypes.byref(n), err, 4096)
        if rc != 0 and b"libhiprtc not found" in err.value:
            pytest.skip("hipRTC not installed")
        assert rc == 0, err.value.decode()
        sizes.append(n.value)
    assert min(sizes) > 10000 and sizes[0] != sizes[1], sizes
