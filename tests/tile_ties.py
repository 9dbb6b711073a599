"""Meshes that aim exact ties in t at the seams of the LDS-tiled scans (schedules 4, 5 and 10;
DESIGN.md §4.2), and the oracle-only measure of whether a frame can show a wrong tie winner.

The tiled scans take the faces in tiles of 256 (kTile), two triangles per step, and the last
triangle of an odd tile alone; the tail form shares a ray's triangles out over several lanes and
merges their nearest hits.  The shader's rule -- at equal t the later face wins
(get_intersection_with_scene :288-295) -- must hold inside a step, between two steps, across a
tile boundary and through every merge.  So each mesh here places stacks of bitwise identical
triangles at chosen face indices; the materials alternate 0 / 1 (white / red) along a stack, so
the face that wins the tie decides the colour of every pixel the stack covers.

Layout: the room (one set of walls) and the light of bvh_adversarial.ties_mesh at faces 0 .. 9;
the stacks, each a right triangle with legs of 35 units facing the camera, in the cells of a
4-column grid in the plane z = 30; small filler triangles at z >= 50, behind the stacks, at every
other index.  Pure numpy, seeded (test infrastructure)."""
import functools

import numpy as np

import bvh_adversarial as A
import oracle as O
import rvcp_amd

f32 = np.float32
TILE = 256                      # kTile (rvcp_kernels.hip)
W, H = 47, 39                   # the GPU test's frame
# ... and its large one, 376 x 312.  The host spreads a small frame over two waves per SIMD, 8
# pixels a wave (static_split), so that every wave of the frames above scans in the tail form
# from its first iteration; here a wave starts with 58 pixels or more -- above the 32 rays at
# which the tail form (or the pool's) takes over -- and runs the scan's two triangles per step.
BIG_SCALE = 8
MIN_SENSITIVE = 10              # pixels that must change when a stack's tie goes the other way

# face count -> ((first face, faces), ...) of the stacks.  Every stack has an even number of
# faces, so that its first and last face differ in material.
STACKS = {
    # 256 k + 1: the last tile is one face, the one "the last triangles of a tile" takes alone
    513: ((20, 4),              # even start: the last two faces share a step
          (41, 4),              # odd start: the last two faces fall in adjacent steps
          (252, 4),             # last face at 255, the last of a tile
          (301, 6),             # odd start in the second tile
          (509, 4)),            # across 511 / 512: last face at 512, alone in its tile, the last of the mesh
    # an odd last tile of 35 faces: steps of two, then face 546 alone
    547: ((30, 4),
          (254, 4),             # across 255 / 256, two faces on each side
          (510, 4),             # across 511 / 512, two faces on each side
          (543, 4)),            # ends on the last face of the odd tile and of the mesh
    # even and no multiple of 256: the last face of the mesh shares its step
    590: ((61, 4),              # odd start
          (253, 4),             # across 255 / 256: last face at 256, the first of a tile
          (384, 6),             # even start in the second tile
          (508, 4),             # last face at 511, the last of a tile
          (586, 4)),            # ends on the last face of the mesh
}
SMALL = 513                     # the mesh the batches and the G-buffer use

# The fuzz scenes of the G-buffer comparison: 17 whose 24 x 20 frame holds at least 60 hits and
# 60 misses (the other scenes' frames are all hits, or all but a few texels: the camera looks
# into a closed room).  Among them the 2^38 offsets (1, 3), 2^37 (16, 30), 2^30 (14) and 2^24
# (5, 8); cameras inside the geometry (1, 5, 6, 8, 10, 11, 16, 17, 25, 28, 30, 32); `dup` in all
# but 18, `coplanar` in all but 1 and 22.
GBUFFER_SEEDS = (1, 3, 4, 5, 6, 8, 10, 11, 14, 16, 17, 18, 22, 25, 28, 30, 32)


def stack_triangle(cell):
    """The triangle of grid cell `cell` (row-major, 4 columns): legs of 35 units in a 40-unit
    cell, each stack in a plane of its own so that no two stacks tie with each other."""
    cx, cy = -60.0 + 40.0 * (cell % 4), 55.0 - 40.0 * (cell // 4)
    z = 30.0 + 0.5 * cell
    return np.array([[cx - 17, cy - 17, z], [cx + 18, cy - 17, z], [cx - 17, cy + 18, z]], f32)


@functools.lru_cache(maxsize=None)
def tile_ties_mesh(n_faces=SMALL, name=None):
    stacks = STACKS[n_faces]
    rng = np.random.default_rng(0x71E5 + n_faces)
    tris = [None] * n_faces
    mats = [0] * n_faces
    room = (A._quad((0, 99, 0), (20, 0, 0), (0, 0, 20)) +
            A._quad((0, -100, 0), (100, 0, 0), (0, 0, 100)) + A._quad((0, 0, 100), (100, 0, 0), (0, 100, 0)) +
            A._quad((-100, 0, 0), (0, 0, 100), (0, 100, 0)) + A._quad((100, 0, 0), (0, 100, 0), (0, 0, 100)))
    for i, t in enumerate(room):
        tris[i], mats[i] = t, 2 if i < 2 else 0
    for cell, (first, n) in enumerate(stacks):
        assert first >= len(room) and n >= 4 and n % 2 == 0 and first + n <= n_faces
        t = stack_triangle(cell)
        for j in range(n):
            assert tris[first + j] is None
            tris[first + j], mats[first + j] = t, j & 1
    for i in range(n_faces):
        if tris[i] is None:         # filler: behind the stacks' planes
            c = np.array([rng.uniform(-90, 90), rng.uniform(-90, 90), rng.uniform(55, 92)])
            tris[i] = (c[None, :] + rng.uniform(-5, 5, (3, 3))).astype(f32)
    return A.Mesh(name or f"tile_ties{n_faces}", np.array(tris, f32), mats, [10, 20, -260], [0, 0, 0],
                  1e-2, t_near=10.0)


def degenerate_alternating_mesh():
    """bvh_adversarial.degenerate_mesh with the materials of its 200 identical faces (192 .. 391,
    across the tile boundary at 256) alternating 0 / 1."""
    return A.degenerate_mesh(alternating=True)


def speck_counts(sc):
    """How many specks (fuzz_scenes._with_specks) a fuzz scene gets for the tiled scans: 230,
    and where that leaves the scene within one tile (20 of the 36 scenes have fewer than 27
    faces) 240 as well, which puts every scene across the boundary at 256."""
    return (230,) if len(sc.mesh.aligned_faces()) + 230 > TILE else (230, 240)


def stack_faces(n_faces):
    """[(first face, last face)] of the mesh's stacks."""
    return [(first, first + n - 1) for first, n in STACKS[n_faces]]


def path_config(mesh):
    """The path-kernel parameters of test_gpu_bvh_adversarial._path_config, without the
    schedule and specialisation fields."""
    return dict(spp=2, ray_t_min=mesh.t_min, ray_t_max=min(4.0 * mesh.diag, A.T_CAP),
                eps=mesh.t_min / 8.0, max_bounces=6)


def oracle_frame(mesh, t, w=W, h=H, mats=None, rect=None):
    """(linear, rgba, traversals) of the CPU oracle for the mesh (with other face materials; of
    the pixels rect = (x0, y0, columns, rows) alone)."""
    from conftest import scene_arrays
    sc = mesh.scene()
    arr = scene_arrays(sc)
    if mats is not None:
        arr["faces"] = arr["faces"].copy()
        arr["faces"]["material_id"] = np.asarray(mats, np.uint32)
        assert np.array_equal(np.flatnonzero(arr["faces"]["material_id"] == 2), arr["lum_face_ids"])
    return O.render(arr, sc.push_constant(t), rvcp_amd.abi.make_config(**path_config(mesh)), w, h, rect=rect)


def swap_mask(mesh, a, b, t=3.0, w=W, h=H, rect=None):
    """bool [rows, columns]: the pixels of the oracle's frame (or of its rect) whose linear bits
    change when faces a and b exchange their materials: what a scan that let a beat b (or b
    beat a) at equal t would show."""
    base = oracle_frame(mesh, t, w, h, rect=rect)[0]
    mats = mesh.mats.copy()
    mats[[a, b]] = mats[[b, a]]
    other = oracle_frame(mesh, t, w, h, mats=mats, rect=rect)[0]
    return np.any(base.view(np.uint32) != other.view(np.uint32), axis=-1)


def swap_sensitivity(mesh, a, b, t=3.0, w=W, h=H, rect=None):
    return int(np.count_nonzero(swap_mask(mesh, a, b, t, w, h, rect)))
