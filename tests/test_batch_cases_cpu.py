"""The conditions on the inputs of tests/test_gpu_batch_matrix.py (tests/batch_cases.py), with
the CPU oracle alone: the frames of a batch differ pairwise, the sky frame is empty and every
other one is not, hits and misses mix where the cases say so, the shard sizes around the
pre-pass threshold are what the GPU tests take them for, and every push is one the host
accepts."""
import numpy as np
import pytest

import batch_cases as B
import rvcp_amd

SAMPLES = B.W * B.H * B.SPP               # 3 666


def _frames(name, pushes, w=B.W, h=B.H):
    return B.oracle_frames(name, B.scene_config(name), pushes, w, h)


def _pairwise_different(frames):
    return all(not np.array_equal(frames[i][1], frames[j][1])
               for i in range(len(frames)) for j in range(i))


def test_cornell_cameras():
    """The figures of the five cameras at 47 x 39, SPP 2, time 3.0."""
    names = B.CORNELL_ORDER + ("inside_a",)
    fr = dict(zip(names, _frames("cornell", [B.push(B.cornell_camera(c), B.TIME) for c in names])))
    assert fr["default"][2] == 15426
    assert fr["inside"][2] == 20220
    assert fr["narrow"][2] == 19914
    assert fr["sky"][2] == SAMPLES
    sky = fr["sky"][1].reshape(-1, 4)
    assert (sky == sky[0]).all()
    # the rolled camera: hits and misses in the same frame (and, 47 pixels a row, the same waves)
    rolled = fr["rolled"][1]
    miss = (rolled == sky[0]).all(-1)
    assert (rolled[0, 0] == sky[0]).all() and int(miss.sum()) == 685 and miss.size == 1833
    cam = B.cornell_camera("rolled")
    # no zero component (right.y is zero for every camera: right = forward x Y)
    assert all(float(x) != 0.0 for v in (cam.position, cam.forward, cam.up, cam.right[::2]) for x in v)
    for name in names:
        if name != "sky":
            assert fr[name][2] > SAMPLES, name
    assert _pairwise_different([fr[n] for n in names])


@pytest.mark.parametrize("name", ["cornell", "c6"])
def test_cornell_batch_frames_differ(name):
    """The batch of the camera tests, in its order and at its times: two frames share a time
    and differ by their cameras, the sky frame sits in the middle."""
    fr = _frames(name, B.cornell_pushes())
    assert _pairwise_different(fr)
    assert B.CORNELL_TIMES[0] == B.CORNELL_TIMES[4] and B.CORNELL_ORDER[2] == "sky"
    for (lin, rgba, trav), cam in zip(fr, B.CORNELL_ORDER):
        assert (trav == SAMPLES) == (cam == "sky"), cam
    assert len(B.scene("c6").mesh.aligned_faces()) == 342


def test_sphere_room_cameras():
    fr = _frames("spheres", B.sphere_pushes())
    assert _pairwise_different(fr)
    for (lin, rgba, trav), cam in zip(fr, B.SPHERE_ORDER):
        assert trav > SAMPLES, cam
    same_time = _frames("spheres", [B.push(c, B.TIME) for c in B.SPHERE_CAMS])
    assert _pairwise_different(same_time)


@pytest.mark.parametrize("seed", B.FUZZ_SEEDS)
def test_fuzz_batches_differ(seed):
    for name in (f"fuzz{seed}", f"fuzz{seed}s"):
        sc, cfg = B.scene(name), B.scene_config(name)
        fr = B.oracle_frames(name, cfg, [sc.push_constant(100.0 + seed + k) for k in range(3)],
                             B.FUZZ_W, B.FUZZ_H)
        assert _pairwise_different(fr), name
        assert all(f[2] > B.FUZZ_W * B.FUZZ_H * cfg["spp"] for f in fr), name


def test_small_frames_differ():
    """9 x 7 x 5 frames and 1 x 1 x 70 frames, the cameras in turn at times 100 + k: the 9 x 7
    frames differ pairwise; of the 70 one-pixel frames (a pixel is one of a few colours; the sphere
    room's is black three times in four) at least ten differ from their neighbour in the queue,
    so a lane that takes its neighbour's frame shows."""
    for name, cams in (("cornell", B.CORNELL_CAMS), ("c6", B.CORNELL_CAMS), ("spheres", B.SPHERE_CAMS)):
        assert _pairwise_different(_frames(name, B.cycled_pushes(cams, 5), 9, 7)), name
        one = _frames(name, B.cycled_pushes(cams, 70), 1, 1)
        colours = [f[0].tobytes() for f in one]
        steps = sum(a != b for a, b in zip(colours, colours[1:]))
        assert len(set(colours)) >= 3 and steps >= 10, \
            f"{name}: {len(set(colours))} colours, {steps} of 69 neighbours differ"


def test_threshold_parsed_and_shard_arithmetic():
    p = B.prepass_batch_max_pixels()
    w = B.THRESHOLD_W
    assert p >= 8 * w and p % (8 * w) == 0      # whole stripes of the threshold frames' width
    h_at, h_above = B.threshold_heights()
    assert h_at * w == p and h_above * w > p
    (h1, k1), (h2, k2) = B.threshold_shards()
    rows = rvcp_amd.shard_rows
    # exactly P pixels on shard 2 of 3, in a slot one stripe larger
    assert rows(h1, k1, 3) * w == p and rows(h1, 0, 3) * w == p + 8 * w
    # more than P pixels on shard 1 of 3, in a slot one more stripe larger
    assert rows(h2, k2, 3) * w == p + 8 * w and rows(h2, 0, 3) * w == p + 16 * w
    assert h1 % 8 == 0 and h2 % 8 == 0 and h2 == h1 + 24
    # the padded shards of group C: 11 stripes, the last of 3 rows
    assert [rows(83, k, 3) for k in range(3)] == [32, 27, 24]
    assert list(rvcp_amd.shard_row_ids(83, 1, 3)[-3:]) == [80, 81, 82]
    # the empty shard
    assert [rows(12, k, 3) for k in range(3)] == [8, 4, 0]
    assert len(rvcp_amd.shard_row_ids(12, 2, 3)) == 0
    # group E's shard 1 of 2
    assert [rows(B.H, k, 2) for k in range(2)] == [23, 16]


def test_every_push_is_in_the_t_range():
    w = B.THRESHOLD_W
    sizes = [(B.W, B.H), (9, 7), (1, 1), (50, 83), (50, 12), (w, B.threshold_heights()[0]),
             (w, B.threshold_heights()[1]), (w, B.threshold_shards()[0][0]), (w, B.threshold_shards()[1][0])]
    for cam in B.CORNELL_CAMS + B.SPHERE_CAMS + (B.cornell_camera("inside_a"),):
        for w_, h_ in sizes:
            assert B.t_range_ok(B.push(cam, 1.0), w_, h_), (cam, w_, h_)
    for seed in B.FUZZ_SEEDS:
        assert B.t_range_ok(B.scene(f"fuzz{seed}").push_constant(1.0), B.FUZZ_W, B.FUZZ_H)
    bad = B.push(B.cornell_camera("default"), 1.0)
    bad["camera"]["t_far"] = 2.0 ** 24
    assert not B.t_range_ok(bad, B.W, B.H)


def test_shard_frames_are_the_rows_of_the_whole():
    """oracle_frames of a shard: the whole frame's rows, and the traversals of the shards of a
    frame add up to the frame's."""
    pushes = B.cornell_pushes()[:2]
    cfg = B.scene_config("cornell")
    whole = B.oracle_frames("cornell", cfg, pushes, 50, 83)
    parts = [B.oracle_frames("cornell", cfg, pushes, 50, 83, k, 3) for k in range(3)]
    for f in range(2):
        assert sum(parts[k][f][2] for k in range(3)) == whole[f][2]
        for k in range(3):
            ids = rvcp_amd.shard_row_ids(83, k, 3)
            assert np.array_equal(parts[k][f][1], whole[f][1][ids])
