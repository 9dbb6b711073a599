"""nonfinite -- inputs and comparisons for the non-finite contract of the post-process kernels
(TEST INFRASTRUCTURE ONLY: never imported by the package).

A texel is live for a launch when it is filterable and every float the launch reads from it is
finite; any other texel is treated exactly as a MISS texel.  So the output for a frame with
poisoned texels equals, bit for bit, the output for the same frame with those texels' face set
to MISS: as_miss() builds that frame, same() compares, salt() poisons.
"""
from __future__ import annotations

import functools

import numpy as np

import denoise_ref as D

F = np.float32
# what salt() writes.  The first three make a texel non-live; the rest are finite and must go
# through the arithmetic as any other value (a subnormal, a signed zero, values whose products
# and sums overflow).
KINDS = {"nan": F(np.nan), "+inf": F(np.inf), "-inf": F(-np.inf), "-0": F(-0.0),
         "subnormal": F(1.0e-45), "+big": F(3.0e38), "-big": F(-3.0e38)}
POISON = ("nan", "+inf", "-inf")
ZERO_NORMAL = "zero_normal"          # a further kind, for fields whose name starts with "normal"
MAX_SHARE = 0.05                     # of the texels, per field


def same(a, b) -> np.ndarray:
    """Elementwise: equal bits, or both NaN (the sign and payload of a generated NaN differ
    between processors, so NaNs are not compared by bits)."""
    a = np.ascontiguousarray(a, dtype=F)
    b = np.ascontiguousarray(b, dtype=F)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what=""):
    bad = ~same(got, want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} words differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}")


def finite(a) -> np.ndarray:
    """[H, W]: no float32 of the texel ([H, W] or [H, W, k]) has an exponent field of all ones.
    Restated here, so the tests do not take the rule from the code they check."""
    a = np.ascontiguousarray(a, dtype=F)
    ok = (a.view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    return ok if a.ndim == 2 else ok.all(axis=-1)


def nonfinite(*arrays) -> np.ndarray:
    """[H, W]: the texels with an infinity or a NaN in any of the arrays ([H, W] or [H, W, k])."""
    out = None
    for a in arrays:
        bad = ~finite(a)
        out = bad if out is None else out | bad
    return out


def gbuffer_nonfinite(g) -> np.ndarray:
    return nonfinite(g["position"], g["normal"])


def as_miss(g, mask):
    """A copy of the G-buffer g with the texels of `mask` turned into MISS texels."""
    out = g.copy()
    out["face"][mask] = D.MISS
    return out


def surrounded(filt) -> np.ndarray:
    """The filterable texels with at least four filterable texels among their eight neighbours."""
    H, W = filt.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = filt
    n = sum(pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
            for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    return filt & (n >= 4)


def salt(arrays, rng, share, filt):
    """Overwrite, in place, a share of the texels of every array of `arrays` (name -> [H, W] or
    [H, W, k] float32: colours, normals, positions, histories, moments, weights) with the values
    of KINDS, one channel of the texel or all of them; an array whose name starts with "normal"
    also gets zero vectors.  `filt` [H, W] (or name -> [H, W]): the filterable texels of the
    frame the array belongs to.  Returns name -> kind -> [H, W] mask of the texels written.

    Asserts that no field has more than MAX_SHARE of its texels written, and that every kind
    landed at least once on a filterable texel with filterable neighbours."""
    assert 0.0 < share <= MAX_SHARE, share
    hits = {}
    for name, a in arrays.items():
        assert a.dtype == F and a.ndim in (2, 3), (name, a.dtype, a.shape)
        H, W = a.shape[:2]
        f = filt[name] if isinstance(filt, dict) else filt
        kinds = list(KINDS) + ([ZERO_NORMAL] if name.startswith("normal") else [])
        n = int(share * H * W)
        assert n >= len(kinds), f"{name}: {W}x{H} holds no {len(kinds)} kinds within {share}"
        good = np.flatnonzero(surrounded(f))
        assert good.size >= len(kinds), f"{name}: too few filterable texels with neighbours"
        first = rng.choice(good, size=len(kinds), replace=False)
        rest = np.setdiff1d(np.arange(H * W), first)
        where = np.concatenate([first, rng.choice(rest, size=n - len(kinds), replace=False)])
        hits[name] = {k: np.zeros((H, W), dtype=bool) for k in kinds}
        for j, t in enumerate(where):
            kind = kinds[j % len(kinds)]
            y, x = divmod(int(t), W)             # (a field of a record array is a strided view)
            if kind == ZERO_NORMAL:
                a[y, x] = 0
            elif a.ndim == 2 or rng.random() < 0.3:
                a[y, x] = KINDS[kind]
            else:
                a[y, x, rng.integers(0, a.shape[2])] = KINDS[kind]
            hits[name][kind][y, x] = True
        written = sum(m for m in hits[name].values())
        assert 0 < written.sum() <= MAX_SHARE * H * W, (name, int(written.sum()))
        for kind, m in hits[name].items():
            assert (m & surrounded(f)).any(), (name, kind)
        for kind in POISON:
            assert (hits[name][kind] & ~finite(a)).any(), (name, kind)
    return hits


def single(a, y, x, kind):
    """A copy of `a` with one texel overwritten: channel 1 (or the value itself) by KINDS[kind],
    the whole vector by zeros for ZERO_NORMAL."""
    out = a.copy()
    if kind == ZERO_NORMAL:
        out[y, x] = 0
    elif out.ndim == 3:
        out[y, x, 1] = KINDS[kind]
    else:
        out[y, x] = KINDS[kind]
    return out


# ------------------------------------------------------------------------ the scene
def zero_normal_scene():
    """The Cornell box plus one triangle at (-30, 250, 200), (30, 250, 200), (0, 300, 200),
    material 0, whose three vertex normals are zero -- the face every OBJ exporter produces
    sooner or later.  It covers no pixel of a 48 x 48 frame, but bounces land on it, and a
    shading normal of zero makes their samples non-finite."""
    import rvcp_amd
    from rvcp_amd import scene as SC
    base = rvcp_amd.Scene.default()
    bv, bf = base.mesh.aligned_vertices(), base.mesh.aligned_faces()
    nv = np.zeros(3, dtype=SC.VERTEX_DTYPE)
    nv["position"][:, :3] = np.array([(-30, 250, 200), (30, 250, 200), (0, 300, 200)], dtype=F)
    nf = np.zeros(1, dtype=SC.FACE_DTYPE)
    nf["vertices"] = len(bv) + np.arange(3, dtype=np.uint32)
    nf["material_id"] = 0
    mesh = SC.ArrayMesh(np.concatenate([bv, nv]), np.concatenate([bf, nf]))
    return SC.Scene(base.camera, list(base.materials), list(base.spheres), mesh)


SCENE_SIZE, SCENE_SPP, SCENE_TIMES = 48, 2, (0.0, 1.0, 2.0, 3.0)


@functools.lru_cache(maxsize=None)
def zero_normal_frames():
    """(scene, G-buffer, [the oracle's linear frames at SCENE_TIMES]) of zero_normal_scene() at
    SCENE_SIZE^2, SCENE_SPP; cached and read-only: the CPU and GPU tests share it."""
    import oracle as O
    import rvcp_amd
    from conftest import scene_arrays
    sc = zero_normal_scene()
    W = H = SCENE_SIZE
    g = D.cpu_gbuffer(sc, W, H)
    g.setflags(write=False)
    frames = []
    for t in SCENE_TIMES:
        lin, _, _ = O.render(scene_arrays(sc), sc.push_constant(t),
                             rvcp_amd.abi.make_config(spp=SCENE_SPP), W, H)
        lin.setflags(write=False)
        frames.append(lin)
    return sc, g, frames
