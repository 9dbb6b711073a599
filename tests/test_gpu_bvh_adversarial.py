"""The opt-in BVH's exactness on adversarial input, on the GPU: the meshes and
cameras of tests/bvh_adversarial.py, every face inside the tree (specialize = OFF gives no
hybrid prefix), ACCEL_BVH against ACCEL_NONE.

  * G-buffer (bvh_nearest<false>, private stack): texels byte-identical, except where the
    classifier excuses them -- the brute-force texel's position lies outside its face's float
    box enlarged by the pad of the builder's formula (less than half a pad inside counts as
    outside).  A texel the BVH hits where the scan misses, or hits nearer than the scan, is
    never excused.  At most 2 % of a frame excused; none at all on the ties, degenerate and
    offset meshes, near or far; the frames must hold hits on duplicated faces, won by the
    higher index.
  * Path kernel (bvh_pool, LDS stacks, carried traversals): linear bits, RGBA8 and traversal
    count equal, no tolerance, on the ties and offset meshes and on every fuzz scene whose
    G-buffer frames had no excused texel.
  * Hybrid: the ties mesh behind the Cornell prefix with copies of prefix faces inside the
    tree, so that a BVH face at equal t must beat a prefix face; specialised module with the
    default t_min, generic prefix scan with ray_t_min = 0.
  * Far cameras, 10 / 100 / 1000 scene diagonals away (wherever t_far x t_coef stays below
    2^24: 33 / 29 / 26 of the 41 meshes): with the traversal's conservative slab comparison
    (kBvhSlabSlack) no texel differs, on any mesh, so none is excused either.

The CPU model of the same traversal (tests/test_bvh_adversarial_cpu.py) is where the planted
faults -- cull tn >= bt, tie rule t < bt, pad zero, a quantised bound rounded inward -- were
tried; this file is the authority for what the model cannot restate, the device's v_rcp_f32 and
its speculative leaf order."""
import functools

import numpy as np
import pytest

import bvh_adversarial as A
import rvcp_amd
from fuzz_scenes import N_FUZZ, fuzz_scene
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W, H = 47, 39                       # odd: the centre pixel has u = v = 0.5 exactly
NEAR = ("camera", "inside", "grazing", "axis")
WELL_FORMED = ["ties", "degenerate"] + [f"offset2^{e}" for e in A.OFFSET_EXPONENTS]


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name.startswith("fuzz"):
        return A.fuzz_mesh(int(name[4:]))
    if name == "ties":
        return A.ties_mesh()
    if name == "degenerate":
        return A.degenerate_mesh()
    return A.offset_mesh(int(name.split("^")[1]))


def _gbuffers(sc, pushes, **kw):
    """The G-buffer of every push constant, from one context; None if the upload reports the
    mesh unsupported (asserted to be that code and no other)."""
    with rvcp_amd.RayTracer(spp=1, specialize=abi.SPECIALIZE_OFF, **kw) as rt:
        try:
            rt.upload_scene(sc)
        except abi.RvcpError as e:
            assert e.code == abi.RVCP_E_UNSUPPORTED, e
            return None
        out = []
        for push in pushes:
            buf = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rt.render_gbuffer_async(push, W, H, buf.data_ptr())
            torch.cuda.synchronize()
            out.append(buf.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W))
        return out


def judge(mesh, cam, a, b):
    """(differing, excused, failures) of BVH frame b against brute-force frame a."""
    diff = np.argwhere((a.view(np.uint8).reshape(H, W, 32) != b.view(np.uint8).reshape(H, W, 32)).any(-1))
    pad_abs = A.builder_pad_abs(mesh.pos)
    o = cam.position.astype(np.float64)
    excused, fails = 0, []
    for y, x in diff:
        ta, tb = a[y, x], b[y, x]
        fa, fb = int(ta["face"]), int(tb["face"])
        if fa == abi.GBUFFER_MISS:
            fails.append((int(y), int(x), "the BVH hits where the scan misses", fa, fb))
            continue
        pa = ta["position"].astype(np.float64)
        if fb != abi.GBUFFER_MISS:
            # not nearer than the scan's hit: distances from the eye, the texels' float32
            # rounding (a few ulp of the largest coordinate per component) allowed for
            pb = tb["position"].astype(np.float64)
            tol = 8.0 * float(np.spacing(np.float32(max(np.abs(pa).max(), np.abs(pb).max(), np.abs(o).max()))))
            if np.linalg.norm(pb - o) < np.linalg.norm(pa - o) - tol:
                fails.append((int(y), int(x), "the BVH's hit is nearer than the scan's", fa, fb))
                continue
        if A.outside_box(mesh.pos, fa, pa, pad_abs):
            excused += 1
        else:
            fails.append((int(y), int(x), "a hit inside its face's enlarged box was lost", fa, fb))
    return len(diff), excused, fails


@functools.lru_cache(maxsize=None)
def gbuffer_report(name):
    """Every camera of the mesh through both contexts: [(kind, differing, excused, failures,
    brute frame, BVH frame)], or None if the BVH upload is unsupported."""
    mesh = mesh_of(name)
    cams = A.gpu_cameras(mesh, per_origin=1)
    sc = mesh.scene()
    pushes = [rvcp_amd.scene.push_constant(c, 0.0) for _, c in cams]
    for p in pushes:            # primary_t_range_ok, by its own formula
        tc = np.sqrt(1.0 + np.tan(np.radians(float(p["camera"]["vertical_fov"]) / 2.0)) ** 2 * (1.0 + (W / H) ** 2))
        assert float(p["camera"]["t_far"]) * tc * 1.001 < 2.0 ** 24
    brute = _gbuffers(sc, pushes, accel=abi.ACCEL_NONE)
    bvh = _gbuffers(sc, pushes, accel=abi.ACCEL_BVH)
    assert brute is not None
    if bvh is None:
        return None
    return [(kind,) + judge(mesh, cam, a, b) + (a, b) for (kind, cam), a, b in zip(cams, brute, bvh)]


ALL = [f"fuzz{s}" for s in range(N_FUZZ)] + WELL_FORMED
NOT_COMPARED = {"unsupported": set(), "path kernel (excused texels)": set()}   # the permitted exits


@pytest.mark.parametrize("name", ALL)
def test_gbuffer_near_and_far(name):
    rep = gbuffer_report(name)
    if rep is None:                 # RVCP_E_UNSUPPORTED, asserted in _gbuffers
        NOT_COMPARED["unsupported"].add(name)
        print(f"{name}: upload unsupported, nothing compared")
        return
    kinds = [r[0] for r in rep]
    assert "camera" in kinds and (name not in WELL_FORMED or {"inside", "grazing", "axis"} <= set(kinds))
    hits = 0
    for kind, ndiff, nexc, fails, a, b in rep:
        print(f"{name} {kind}: hits {int((a['face'] != abi.GBUFFER_MISS).sum())} differing {ndiff} excused {nexc}")
        hits += int((a["face"] != abi.GBUFFER_MISS).sum())
        assert not fails, f"{name} {kind}: {len(fails)} unexcused texels, first {fails[0]}"
        assert nexc <= 0.02 * W * H, f"{name} {kind}: {nexc} excused texels"
        if kind in A.FAR:               # the slack's promise: nothing excused from afar, on any mesh
            assert ndiff == 0, f"{name} {kind}: {ndiff} texels differ ({nexc} excused)"
        if name in WELL_FORMED:         # and every frame sees the mesh
            assert ndiff == 0, f"{name} {kind}: {ndiff} texels differ"
            assert (a["face"] != abi.GBUFFER_MISS).sum() >= 50, f"{name} {kind}: an empty frame"
    assert hits >= 200, f"{name}: {hits} hits in {len(rep)} frames"
    if name == "ties" or name.startswith("offset"):
        mesh = mesh_of(name)
        up = mesh.upper_duplicates()
        keys = [p.tobytes() for p in mesh.pos]
        copied = {keys[i] for i in np.flatnonzero(up)}
        has_copy = np.array([k in copied for k in keys]) & ~up
        for kind, _, _, _, a, b in rep:
            f = b["face"][b["face"] != abi.GBUFFER_MISS]
            assert not has_copy[f].any(), f"{name} {kind}: a lower-indexed copy won a tie"
        won = sum(int(up[b["face"][b["face"] != abi.GBUFFER_MISS]].sum()) for *_, b in rep)
        assert won >= 1000, f"{name}: only {won} texels on the later copy of a duplicated face"


def test_far_cameras_share():
    """Share of excused texels per camera distance over all meshes (recorded in DESIGN.md
    §4.6); the per-frame assertions are test_gbuffer_near_and_far's."""
    tot = {}
    for name in ALL:
        rep = gbuffer_report(name)
        for kind, ndiff, nexc, fails, a, b in rep or []:
            t = tot.setdefault(kind, [0, 0, 0])
            t[0] += nexc
            t[1] += ndiff
            t[2] += 1
    for kind, (nexc, ndiff, frames) in tot.items():
        print(f"{kind}: {frames} frames, {ndiff} differing, {nexc} excused texels "
              f"({100.0 * nexc / (frames * W * H):.4f} %)")
    for kind in A.FAR:          # (the larger offset meshes cannot be seen from that far: 2^24)
        assert tot[kind][2] >= 20 and tot[kind][1] == 0 and tot[kind][0] == 0, (kind, tot[kind])


def _render(sc, t, **kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(sc)
        rgba, lin = rt.render(W, H, t, want_linear=True)
        return rgba, lin, rt.last_stats.copy()


def _same(sc, t, **kw):
    a = _render(sc, t, **kw)
    b = _render(sc, t, accel=abi.ACCEL_BVH, **kw)
    diff = np.any(a[1].view(np.uint32) != b[1].view(np.uint32), axis=-1)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ"
    assert np.array_equal(a[0], b[0])
    assert int(a[2]["traversals"]) == int(b[2]["traversals"])
    assert int(a[2]["traversals"]) > W * H
    return a, b


def _path_config(mesh):
    return dict(spp=2, ray_t_min=mesh.t_min, ray_t_max=min(4.0 * mesh.diag, A.T_CAP),
                eps=mesh.t_min / 8.0, max_bounces=6, specialize=abi.SPECIALIZE_OFF)


@pytest.mark.parametrize("name", ["ties"] + [f"offset2^{e}" for e in A.OFFSET_EXPONENTS])
def test_path_kernel_ties(name):
    mesh = mesh_of(name)
    _same(mesh.scene(), 3.0, **_path_config(mesh))


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_path_kernel_fuzz(seed):
    """Every fuzz scene whose G-buffer frames had no excused texel (a scene where the exact
    test reports hits far outside a sliver face cannot promise equal frames)."""
    rep = gbuffer_report(f"fuzz{seed}")
    if rep is None or any(r[2] for r in rep):
        NOT_COMPARED["path kernel (excused texels)" if rep else "unsupported"].add(f"fuzz{seed}")
        print(f"fuzz{seed}: path kernel not compared")
        return
    sc, kw, desc = fuzz_scene(seed)
    _same(sc, 100.0 + seed, specialize=abi.SPECIALIZE_OFF, **kw)


def test_what_was_not_compared():
    """The exits the issue permits -- an unsupported upload, a fuzz scene with excused G-buffer
    texels left out of the path-kernel comparison -- named, and held to a minority: every
    mesh here is built to be legal input and the model excuses under 0.1 % of its rays, so a
    run in which half of the scenes leave by an exit compares too little to mean anything."""
    for name in ALL:
        if gbuffer_report(name) is None:
            NOT_COMPARED["unsupported"].add(name)
    for seed in range(N_FUZZ):
        rep = gbuffer_report(f"fuzz{seed}")
        if rep is not None and any(r[2] for r in rep):
            NOT_COMPARED["path kernel (excused texels)"].add(f"fuzz{seed}")
    for why, names in NOT_COMPARED.items():
        print(f"not compared, {why}: {sorted(names) or 'none'}")
    assert not NOT_COMPARED["unsupported"] & set(WELL_FORMED)
    assert len(NOT_COMPARED["unsupported"]) + len(NOT_COMPARED["path kernel (excused texels)"]) <= N_FUZZ // 2


def _hybrid_scene(cornell):
    """Cornell's 32 faces (the prefix), the ties mesh inside the room, and copies of the first
    twelve Cornell faces (the room) at the end, inside the tree."""
    mesh = A.ties_mesh()
    bv, bf = cornell.mesh.aligned_vertices(), cornell.mesh.aligned_faces()
    n = len(mesh.pos)
    nv = np.zeros(3 * n, bv.dtype)
    nv["position"][:, :3] = (mesh.pos.reshape(-1, 3) + np.float32([0, 274, 0])).astype(np.float32)
    nv["normal"][:, 1] = 1.0
    nf = np.zeros(n, bf.dtype)
    nf["vertices"] = len(bv) + np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    copies = bf[:12].copy()           # light, top, left, right, front, bottom
    faces = np.concatenate([bf, nf, copies])
    return rvcp_amd.Scene(cornell.camera, cornell.materials, [],
                          rvcp_amd.scene.ArrayMesh(np.concatenate([bv, nv]), faces)), len(faces)


def test_hybrid_prefix_ties(cornell):
    sc, n = _hybrid_scene(cornell)
    _, b = _same(sc, 3.5, spp=2)
    assert int(b[2]["kernel_variant"]) & abi.VARIANT_SPECIALIZED
    _, b = _same(sc, 3.5, spp=2, ray_t_min=0.0)
    assert not int(b[2]["kernel_variant"]) & abi.VARIANT_SPECIALIZED
    # the G-buffer of the hybrid context: the copies in the tree beat their prefix originals
    push = [sc.push_constant(0.0)]
    with rvcp_amd.RayTracer(spp=1, accel=abi.ACCEL_BVH) as rt:
        rt.upload_scene(sc)
        buf = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rt.render_gbuffer_async(push[0], W, H, buf.data_ptr())
        torch.cuda.synchronize()
        g = buf.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W)
    ref = _gbuffers(sc, push, accel=abi.ACCEL_NONE)[0]
    assert g.tobytes() == ref.tobytes()
    f = g["face"][g["face"] != abi.GBUFFER_MISS]
    assert (f >= n - 12).sum() >= 100 and not (f < 12).any()
