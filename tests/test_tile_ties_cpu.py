"""Conditions on the inputs of tests/test_gpu_schedules_adversarial.py, checked with the CPU
oracle alone (no GPU): the tile-ties meshes of tests/tile_ties.py put their stacks where the
tiled scans have their seams, and a wrong tie winner in any stack would show in the frame the
GPU test compares.  These are conditions on the inputs, not tolerances on any kernel."""
import numpy as np
import pytest

import bvh_adversarial as A
import tile_ties as T
from fuzz_scenes import N_FUZZ, _with_specks, fuzz_scene


@pytest.mark.parametrize("n_faces", sorted(T.STACKS))
def test_stack_layout(n_faces):
    m = T.tile_ties_mesh(n_faces)
    assert len(m.pos) == n_faces == len(m.mats)
    ties = A.ties_mesh()
    assert np.array_equal(m.pos[:2], ties.pos[:2]) and np.array_equal(m.pos[2:10], ties.pos[22:30])
    assert np.array_equal(m.cam_pos, ties.cam_pos) and np.array_equal(m.look, ties.look)
    in_stack = np.zeros(n_faces, bool)
    for first, last in T.stack_faces(n_faces):
        assert last - first + 1 >= 4 and first >= 10
        for j in range(first, last + 1):
            assert m.pos[j].tobytes() == m.pos[first].tobytes()      # bitwise identical
            assert int(m.mats[j]) == (j - first) & 1                 # 0 / 1 in turn
        assert int(m.mats[first]) != int(m.mats[last])
        in_stack[first:last + 1] = True
    # the filler lies behind every stack, and nothing else repeats a face
    z = m.pos[:, :, 2]
    assert z[in_stack].max() < z[10:][~in_stack[10:]].min()
    assert int(m.upper_duplicates().sum()) == sum(l - f for f, l in T.stack_faces(n_faces))


def test_stack_positions_cover_the_seams():
    """Every position the tiled scans treat differently holds the end of a stack in some mesh."""
    assert any(n % T.TILE == 1 for n in T.STACKS)
    assert any(n % 2 == 0 and n % T.TILE != 0 for n in T.STACKS)
    seen = set()
    for n in T.STACKS:
        last_tile = (n - 1) // T.TILE * T.TILE
        for first, last in T.stack_faces(n):
            tile_first, tile_last = first // T.TILE, last // T.TILE
            if tile_first == tile_last and first % 2 == 0:
                seen.add("even start: the last two faces share a step")
            if tile_first == tile_last and first % 2 == 1:
                seen.add("odd start: the last two faces in adjacent steps")
            for edge in (256, 512):
                if last == edge - 1:
                    seen.add(f"last face at {edge - 1}")
                if last == edge:
                    seen.add(f"last face at {edge}")
                if first < edge - 1 and last > edge:
                    seen.add(f"two faces on each side of {edge - 1} / {edge}")
            if last == n - 1:
                seen.add("last face of the mesh")
                if (n - last_tile) % 2 == 1:
                    seen.add("last face of an odd last tile")
                    if n - last_tile > 1:
                        seen.add("last face of an odd last tile after whole steps")
                else:
                    seen.add("last face of the mesh shares its step")
    want = {"even start: the last two faces share a step", "odd start: the last two faces in adjacent steps",
            "last face at 255", "last face at 256", "last face at 511", "last face at 512",
            "two faces on each side of 255 / 256", "two faces on each side of 511 / 512",
            "last face of the mesh", "last face of an odd last tile",
            "last face of an odd last tile after whole steps", "last face of the mesh shares its step"}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("n_faces", sorted(T.STACKS))
def test_every_stack_shows_its_tie_winner(n_faces):
    """Exchange the materials of a stack's last two faces, and of its first and last: the
    oracle's frame at the GPU test's size and config changes on at least 10 pixels, so a scan
    that let another face of the stack win the tie cannot pass the GPU comparison."""
    m = T.tile_ties_mesh(n_faces)
    k = T.BIG_SCALE
    for first, last in T.stack_faces(n_faces):
        mask = T.swap_mask(m, last - 1, last)
        two, ends = int(mask.sum()), T.swap_sensitivity(m, first, last)
        # the large frame has the small one's camera and k x k pixels for each of its pixels:
        # there the oracle renders the 3 x 3 small pixels around the median of those that
        # changed above (the stack itself; a few more change by the light it reflects)
        ys, xs = np.nonzero(mask)
        x0 = min(max(int(np.median(xs)) - 1, 0), T.W - 3)
        y0 = min(max(int(np.median(ys)) - 1, 0), T.H - 3)
        rect = (k * x0, k * y0, 3 * k, 3 * k)
        big_two = T.swap_sensitivity(m, last - 1, last, w=k * T.W, h=k * T.H, rect=rect)
        big_ends = T.swap_sensitivity(m, first, last, w=k * T.W, h=k * T.H, rect=rect)
        print(f"tile_ties{n_faces} stack {first} .. {last}: last two {two} pixels, first and last {ends} pixels"
              f" at {T.W} x {T.H}; {big_two} and {big_ends} at {k * T.W} x {k * T.H}")
        assert min(two, ends, big_two, big_ends) >= T.MIN_SENSITIVE, (n_faces, first, last)


def test_degenerate_run_alternates():
    """The alternating variant differs from degenerate_mesh in the run's materials alone; its
    frame shows the winner of the run, which the one-material mesh cannot."""
    old, new = A.degenerate_mesh(), T.degenerate_alternating_mesh()
    assert old.name == "degenerate" and new.name == "degenerate_alt"
    assert old.pos.tobytes() == new.pos.tobytes()
    run = np.arange(192, 392)
    assert all(old.pos[j].tobytes() == old.pos[192].tobytes() for j in run)
    assert (old.mats[run] == 1).all() and np.array_equal(new.mats[run], (run - 192) & 1)
    other = np.setdiff1d(np.arange(len(old.mats)), run)
    assert np.array_equal(old.mats[other], new.mats[other])
    two = T.swap_sensitivity(new, 390, 391)
    ends = T.swap_sensitivity(new, 192, 391)
    same = T.swap_sensitivity(old, 390, 391)
    print(f"degenerate_alt run 192 .. 391: last two {two} pixels, first and last {ends} pixels; "
          f"degenerate: {same}")
    assert two >= T.MIN_SENSITIVE and ends >= T.MIN_SENSITIVE and same == 0


def test_gbuffer_seeds_cover_the_cases():
    """The G-buffer seeds, read off each scene's description: every 2^38 offset, a camera
    inside the geometry, a scene with `dup` and one with `coplanar`."""
    descs = [fuzz_scene(s)[2] for s in T.GBUFFER_SEEDS]
    every = [fuzz_scene(s)[2] for s in range(N_FUZZ)]
    assert len(set(T.GBUFFER_SEEDS)) >= 12
    assert sum("offset 2^38" in d for d in descs) == sum("offset 2^38" in d for d in every) >= 2
    for word in ("camera inside", "'dup'", "'coplanar'"):
        assert any(word in d for d in descs), word


def test_specks_cross_one_tile_boundary():
    """The speck counts of the GPU test's tile-boundary case: 230 leaves the scenes of fewer
    than 27 faces inside one tile (250 .. 256 faces), so those get 240 as well."""
    crossing = 0
    for seed in range(N_FUZZ):
        sc = fuzz_scene(seed)[0]
        counts = [len(_with_specks(sc, n, seed).mesh.aligned_faces()) for n in T.speck_counts(sc)]
        assert counts[0] == len(sc.mesh.aligned_faces()) + 230
        assert T.TILE < counts[-1] <= 2 * T.TILE, (seed, counts)
        crossing += counts[0] > T.TILE
    assert 0 < crossing < N_FUZZ        # both a nearly full single tile and a crossing at 230
