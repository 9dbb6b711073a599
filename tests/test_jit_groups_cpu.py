"""The grouped scan of rvcp_jit.cpp (DESIGN.md §4.7 "Face groups"), checked on the CPU.

A games101 scene's faces are split into an always set and face groups; a ray tests a group only
when it reaches the group's padded box over [t_min, its bound] or runs nearly parallel to one of
the group's planes.  The cull may never drop a (ray, face) pair the full scan accepts, so the
generated grouped text is compiled with g++ (tests/spec_groups.py) and four things are compared
bit for bit on t, face and the shadow slot's hit flag, for every ray that passes the kernel's
per-wave guard:

    the grouped scan                                (slab reciprocal = the IEEE quotient)
    the model: the same with the reciprocal moved by +1 and by -1 ulp (v_rcp_f32 is within 1 ulp)
    the ungrouped generated scan
    a reference loop in the numeric contract's operation order

Scenes: the Cornell box, scene.rotated_scene, Cornell plus a third box (42 faces, three groups), the
overflow scene of the GPU test and every fuzz scene of tests/fuzz_scenes.py.  Rays per scene: 10^6
random ones (origins in and around the scene box and on the faces, directions uniform with exact
zeros mixed in) and the classes of tests/bvh_adversarial.py started from points on and just off
every face: aimed at vertices and edge midpoints, grazing (in the face's plane plus 10^-2 .. 10^-6
of the normal) and axis-parallel with one and two exact-zero components.

Tolerance: none.  Zero mismatches."""
import numpy as np
import pytest

import rvcp_amd
from fuzz_scenes import N_FUZZ, fuzz_scene
from spec_groups import GroupedScan, crowded_scene, partition, positions, three_box_scene
from test_jit_cpu import _norm, _tri_records

f32 = np.float32
N_RANDOM = 1_000_000
HEIGHT = 0.25        # rvcp_jit.cpp kGroupHeight: a group's faces are at least this well conditioned


def _random_rays(pos, rng, n):
    """Origins: a third in the scene box grown by a quarter, two thirds on faces (area-weighted
    barycentric points, half of them lifted off the face by 2^-12 .. 2^-4 of the scene's extent
    along +- the normal).  Directions: uniform; a sixth with one exact-zero component, a twelfth
    with two."""
    p = pos.astype(np.float64)
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    k = n // 3
    o = np.empty((n, 3))
    o[:k] = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (k, 3))
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    ok = np.isfinite(area) & (area > 0)
    w = np.where(ok, area, 0.0)
    f = rng.choice(len(p), n - k, p=w / w.sum())
    b = rng.dirichlet([1.0, 1.0, 1.0], n - k)
    o[k:] = np.einsum("rk,rkc->rc", b, p[f])
    lift = rng.choice([0.0, 1.0], n - k) * rng.choice([-1.0, 1.0], n - k) * ext * 2.0 ** -rng.integers(4, 13, n - k)
    o[k:] += (nrm[f] / area[f, None]) * lift[:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    z = n // 6
    d[np.arange(z), rng.integers(0, 3, z)] = 0.0
    z2 = n // 12
    keep = rng.integers(0, 3, z2)
    for a in range(3):
        d[z:z + z2, a] = np.where(keep == a, np.sign(d[z:z + z2, a]) + (d[z:z + z2, a] == 0), 0.0)
    return np.concatenate([o.astype(f32), d.astype(f32)], axis=1)


def _adversarial_rays(pos, rng, per_face=6):
    """From `per_face` points on every face with a non-zero area, each also lifted off the face by
    2^-14 of the scene's extent on either side: rays aimed at a vertex and at an edge midpoint of a
    random face and of the face's own group neighbour (the next face), grazing rays (in the
    origin face's plane plus 10^-2 .. 10^-6 of its normal, and grazing a random other face's plane
    through one of that face's vertices and edge midpoints), and axis-parallel rays with two
    exact-zero components and with one."""
    p = pos.astype(np.float64)
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    good = np.flatnonzero(np.isfinite(area) & (area > 0))
    unit = nrm[good] / area[good, None]
    rays = []
    for gi, fidx in enumerate(good):
        n_hat = unit[gi]
        for _ in range(per_face):
            q = rng.dirichlet([1.0, 1.0, 1.0]) @ p[fidx]
            for off in (0.0, ext * 2.0 ** -14, -ext * 2.0 ** -14):
                o = (q + off * n_hat).astype(f32)
                of = o.astype(np.float64)
                for tf in (int(rng.choice(good)), int(good[(gi + 1) % len(good)])):
                    v = p[tf]
                    kk = int(rng.integers(0, 3))
                    for tgt in (v[kk], 0.5 * (v[kk] + v[(kk + 1) % 3])):
                        dv = tgt - of
                        if np.linalg.norm(dv) > 0:
                            rays.append(np.concatenate([o, (dv / np.linalg.norm(dv)).astype(f32)]))
                    # grazing the target face's plane: from a point of that plane half an extent
                    # from the target, lifted by 10^-2 .. 10^-6 of that distance
                    tn = np.cross(v[1] - v[0], v[2] - v[0])
                    tn /= np.linalg.norm(tn)
                    a = np.cross(tn, rng.normal(size=3))
                    a /= np.linalg.norm(a)
                    tgt = v[kk] if rng.random() < 0.5 else 0.5 * (v[kk] + v[(kk + 1) % 3])
                    og = (tgt + 0.5 * ext * a + 0.5 * ext * tn * 10.0 ** -rng.integers(2, 7)).astype(f32)
                    dv = tgt - og.astype(np.float64)
                    rays.append(np.concatenate([og, (dv / np.linalg.norm(dv)).astype(f32)]))
                # grazing the origin's own face
                a = np.cross(n_hat, rng.normal(size=3))
                a /= np.linalg.norm(a)
                dg = a + n_hat * rng.choice([-1.0, 1.0]) * 10.0 ** -rng.integers(2, 7)
                rays.append(np.concatenate([o, (dg / np.linalg.norm(dg)).astype(f32)]))
                # axis-parallel: two exact zeros, then one
                ax = int(rng.integers(0, 3))
                d2 = np.zeros(3)
                d2[ax] = rng.choice([-1.0, 1.0])
                rays.append(np.concatenate([o, d2.astype(f32)]))
                d1 = rng.normal(size=3)
                d1[ax] = 0.0
                rays.append(np.concatenate([o, (d1 / np.linalg.norm(d1)).astype(f32)]))
    return np.array(rays, f32)


def _compare(gs, rays, tmin, tmax, what):
    """Zero mismatches between the four scans on `rays`; returns (rays that passed the guard,
    pairs, pairs culled)."""
    base = None
    for mode in (0, 1, -1):
        t, face, flags, counts = gs.run(rays, tmin, tmax, mode)
        tb = t.view(np.uint32)
        # the ungrouped scan against the reference loop (where the ungrouped scan's own premise,
        # ray_in_range, holds)
        in_range, passed = (flags & 2) != 0, (flags & 1) != 0
        bad = in_range & ((tb[:, 3] != tb[:, 4]) | (face[:, 1] != face[:, 2]))
        assert not bad.any(), (what, "ungrouped != reference", rays[bad][:3].tolist())
        if gs.n_groups:
            bad = passed & ((tb[:, 0] != tb[:, 4]) | (face[:, 0] != face[:, 2]))
            assert not bad.any(), (what, mode, "grouped path slot != reference", int(bad.sum()),
                                   rays[bad][:3].tolist(), t[bad][:3].tolist(), face[bad][:3].tolist())
            # the shadow slot: its t, and with it the hit flag (t != t_max), and slot B of the dual form
            bad = passed & ((tb[:, 1] != tb[:, 4]) | (tb[:, 2] != tb[:, 4]))
            assert not bad.any(), (what, mode, "grouped dual scan != reference", int(bad.sum()),
                                   rays[bad][:3].tolist())
        if base is None:
            base = counts
    return base


def _check_scene(tmp_path, sc, name, tmin, tmax, seed):
    gs = GroupedScan(tmp_path, sc, name)
    rng = np.random.default_rng(0x6A0 + seed)
    counts = _compare(gs, _random_rays(gs.pos, rng, N_RANDOM), tmin, tmax, name + " random")
    _compare(gs, _adversarial_rays(gs.pos, rng), tmin, tmax, name + " adversarial")
    return gs, counts


def test_cornell_partition_and_cull(tmp_path):
    sc = rvcp_amd.Scene.default()
    gs, counts = _check_scene(tmp_path, sc, "cornell", 0.01, 10000.0, 0)
    group_of, box = partition(gs.rec, gs.mask)
    assert group_of[:12].tolist() == [-1] * 12
    assert group_of[12:22].tolist() == [0] * 10 and group_of[22:32].tolist() == [1] * 10
    assert gs.n_groups == 2 and len(box) == 2
    # the padded boxes hold their faces
    for g in range(2):
        p = gs.pos[group_of == g].reshape(-1, 3)
        assert np.all(p >= box[g, 0]) and np.all(p <= box[g, 1])
    passed, pairs, culled = (int(c) for c in counts)
    print(f"cornell: {passed} of {N_RANDOM} random rays pass the guard; {culled} of {pairs} "
          f"(ray, group) pairs culled ({culled / pairs:.3f})")
    assert passed >= 0.9 * N_RANDOM
    assert culled >= 0.5 * pairs


def test_rotated_cornell(tmp_path):
    sc = rvcp_amd.scene.rotated_scene(rvcp_amd.Scene.default())
    _check_scene(tmp_path, sc, "rotated", 0.01, 10000.0, 1)


def test_three_groups(tmp_path):
    gs, counts = _check_scene(tmp_path, three_box_scene(), "threebox", 0.01, 10000.0, 2)
    group_of, _ = partition(gs.rec, gs.mask)
    assert len(gs.pos) == 42 and gs.n_groups == 3
    assert group_of[32:].tolist() == [2] * 10 and group_of[:12].tolist() == [-1] * 12


def test_crowded_scene_overflows_a_pass(tmp_path):
    """The GPU suite's overflow scene: three groups, and the rays of a steady-state wave (about
    64 shadow and 50 path rays) reach more (ray, group) pairs than the 64 of one
    pass -- on this ray model, more than 64 / 114 pairs per ray."""
    gs, counts = _check_scene(tmp_path, crowded_scene(), "crowded", 0.01, 10000.0, 3)
    assert gs.n_groups == 3
    passed, pairs, culled = (int(c) for c in counts)
    print(f"crowded: {(pairs - culled) / passed:.3f} pairs reached per ray")
    assert (pairs - culled) / passed > 64.0 / 114.0


def _ill_conditioned(pos):
    p = pos.astype(np.float64)
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 2] - p[:, 1]], axis=1)
    longest2 = (e ** 2).sum(-1).max(-1)
    area2 = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
    with np.errstate(invalid="ignore"):
        return ~(area2 >= HEIGHT * longest2) | ~(longest2 > 0)


@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzz_scenes(tmp_path, seed):
    sc, kw, desc = fuzz_scene(seed)
    gs, _ = _check_scene(tmp_path, sc, f"fuzz{seed}", float(f32(kw["ray_t_min"])),
                         float(f32(kw["ray_t_max"])), 10 + seed)
    group_of, _ = partition(gs.rec, gs.mask)
    bad = _ill_conditioned(gs.pos)
    assert np.all(group_of[bad] == -1), desc
    assert (gs.text == "") == (gs.n_groups == 0)


def test_no_group_no_text():
    """A scene without an eligible group gets today's module: no grouped text at all."""
    sc, _, _ = fuzz_scene(0)
    rec = _tri_records(positions(sc))
    group_of, box = partition(rec, 0)
    if np.all(group_of == -1):
        from spec_groups import groups_source
        assert groups_source(rec, 0) == "" and len(box) == 0
    # the Cornell box with every box face marked luminous: the light stays in the always set
    cp = positions(rvcp_amd.Scene.default())
    group_of, _ = partition(_tri_records(cp), (1 << 32) - 1)
    assert np.all(group_of == -1)
