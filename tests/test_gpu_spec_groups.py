"""The grouped scan on the GPU (DESIGN.md §4.7 "Face groups"): frames of scenes whose specialised
module tests its face groups only for the rays that reach them, against the CPU oracle.

    linear RGB bits equal, RGBA8 bytes equal, `traversals` equal; nothing excused.

Every case asserts the schedule that ran and its VARIANT_SPECIALIZED bit, and that the frame is
not empty.  tests/test_jit_groups_cpu.py holds the conditions on the inputs: that these scenes
have the groups the cases are about (the Cornell box two, the three-box scenes three) and that the
overflow scene's rays reach more (ray, group) pairs per wave than one pass of 64 holds.

Frame sizes (tests/test_gpu_schedules_adversarial.py): 48 x 40 frames run in the compact and
tail forms; 416 x 320 is the smallest size at which a wave starts with 64 pixels and so reaches the
dual scan.  The cosine build has no oracle; its reference is schedule 1's generic kernel in cosine
mode, as in tests/test_gpu_importance.py."""
import functools

import numpy as np
import pytest

import oracle as O
import rvcp_amd
from conftest import scene_arrays
from rvcp_amd import abi
from spec_groups import crowded_scene, three_box_scene

pytestmark = pytest.mark.gpu
SPEC = abi.VARIANT_SPECIALIZED
OFF = abi.SPECIALIZE_OFF
SMALL, BIG = (48, 40, 4), (416, 320, 2)        # width, height, SPP
TIME = 123.0


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "cornell":
        return rvcp_amd.Scene.default()
    if name == "rotated":
        return rvcp_amd.scene.rotated_scene(rvcp_amd.Scene.default())
    if name == "threebox":
        return three_box_scene()
    assert name == "crowded"
    return crowded_scene()


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp, t=TIME):
    sc = _scene(name)
    orc = O.render(scene_arrays(sc), sc.push_constant(t), abi.make_config(spp=spp), w, h)
    for a in orc[:2]:
        a.setflags(write=False)
    return orc


def _gpu(sc, w, h, t, **kw):
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(sc)
        rgba, lin = rt.render(w, h, t, want_linear=True)
        return rgba, lin, rt.last_stats.copy()


def _compare(problems, label, got, ref, variant, samples):
    rgba, lin, stats = got
    r_lin, r_rgba, r_trav = ref
    kv = int(stats["kernel_variant"])
    if kv & 15 != variant or not kv & SPEC:
        problems.append(f"{label}: kernel_variant {kv}, wanted schedule {variant}, specialised")
    if not int(r_trav) > samples:
        problems.append(f"{label}: an empty frame, {r_trav} traversals of {samples} samples")
    diff = np.any(lin.view(np.uint32) != r_lin.view(np.uint32), axis=-1)
    if diff.any():
        problems.append(f"{label}: {int(diff.sum())} pixels differ in linear RGB, first at "
                        f"{np.argwhere(diff)[:3].tolist()}")
    if not np.array_equal(rgba, r_rgba):
        problems.append(f"{label}: {int(np.any(rgba != r_rgba, axis=-1).sum())} pixels differ in RGBA8")
    if int(stats["traversals"]) != int(r_trav):
        problems.append(f"{label}: traversals {int(stats['traversals'])}, wanted {int(r_trav)}")


@pytest.mark.parametrize("size", [SMALL, BIG], ids=["48x40", "416x320"])
@pytest.mark.parametrize("variant", [3, 6])
@pytest.mark.parametrize("name", ["cornell", "rotated"])
def test_schedules_against_the_oracle(name, variant, size):
    w, h, spp = size
    problems = []
    got = _gpu(_scene(name), w, h, TIME, kernel_variant=variant, spp=spp)
    _compare(problems, f"{name} schedule {variant} {w}x{h}", got, _oracle(name, w, h, spp), variant, w * h * spp)
    assert not problems, problems


def test_three_groups():
    w, h, spp = SMALL
    problems = []
    for v in (3, 6):
        got = _gpu(_scene("threebox"), w, h, TIME, kernel_variant=v, spp=spp)
        _compare(problems, f"three boxes schedule {v}", got, _oracle("threebox", w, h, spp), v, w * h * spp)
    assert not problems, problems


def test_more_items_than_one_pass():
    """The overflow loop: full waves of the crowded scene hold more than 64 (ray, group) pairs
    (tests/test_jit_groups_cpu.py::test_crowded_scene_overflows_a_pass), scanned in two passes."""
    w, h, spp = BIG
    problems = []
    for v in (3, 6):
        got = _gpu(_scene("crowded"), w, h, TIME, kernel_variant=v, spp=spp)
        _compare(problems, f"crowded schedule {v}", got, _oracle("crowded", w, h, spp), v, w * h * spp)
    assert not problems, problems


def test_cosine_build():
    """The cosine-sampling module shares path_body: schedules 3 and 6 specialised against
    schedule 1's generic kernel, both in cosine mode."""
    w, h, spp = SMALL
    sc = _scene("cornell")

    def cos(**kw):
        with rvcp_amd.RayTracer(spp=spp, **kw) as rt:
            rt.sampling = abi.SAMPLING_COSINE
            rt.upload_scene(sc)
            rgba, lin = rt.render(w, h, TIME, want_linear=True)
            return rgba, lin, rt.last_stats.copy()

    ref = cos(kernel_variant=1, specialize=OFF)
    assert not int(ref[2]["kernel_variant"]) & SPEC
    problems = []
    for v in (3, 6):
        _compare(problems, f"cosine schedule {v}", cos(kernel_variant=v),
                 (ref[1], ref[0], int(ref[2]["traversals"])), v, w * h * spp)
    assert not problems, problems


def test_spp_map_build():
    """The per-pixel sample-count module shares path_body: a random map of the levels 1 .. 16
    against the oracle's frames of each level."""
    from test_gpu_spp_map import check, expected, map_render, random_map
    w, h = 48, 40
    m = random_map(w, h)
    want_rgba, want_lin = expected("cornell", w, h, m)
    problems = []
    for v in (3, 6):
        check(problems, f"map schedule {v}", map_render(_scene("cornell"), w, h, 123.0, m, kernel_variant=v),
              want_rgba, want_lin, m, v, True)
    assert not problems, problems


def test_batch_with_per_frame_cameras():
    """Three frames in one launch (rvcp_render_frames_async), each with its own time and the last
    with a moved camera: every frame is the oracle's frame of its push constant."""
    torch = pytest.importorskip("torch")
    w, h, spp = SMALL
    sc = _scene("cornell")
    pushes = [sc.push_constant(t) for t in (TIME, 7.5, 31.0)]
    pushes[2]["camera"]["position"][0] += 7.0
    out = torch.zeros((3, h, w), dtype=torch.int32, device="cuda")
    with rvcp_amd.RayTracer(spp=spp) as rt:
        rt.upload_scene(sc)
        rt.render_frames_async(pushes, w, h, 0, 1, out.data_ptr())
        st = rt.sync_stats()
        torch.cuda.synchronize()
    assert int(st["kernel_variant"]) & SPEC
    got = out.cpu().numpy().view(np.uint8).reshape(3, h, w, 4)
    trav = 0
    for k, p in enumerate(pushes):
        _, o_rgba, o_trav = O.render(scene_arrays(sc), p, abi.make_config(spp=spp), w, h)
        assert np.array_equal(got[k], o_rgba), f"batch frame {k} differs from the oracle"
        trav += int(o_trav)
    assert int(st["traversals"]) == trav
