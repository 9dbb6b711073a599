"""The packed item layout of the grouped scan on the GPU (csrc/rvcp_group_pack.h, spec_group_pass;
DESIGN.md §4.7 "Face groups"): frames whose waves hold one group's items in passes of their own,
padding before a group and a group spanning two passes, against the CPU oracle.

    linear RGB bits equal, RGBA8 bytes equal, `traversals` equal; nothing excused

(the comparison of tests/test_gpu_spec_groups.py).  tests/test_group_pack_cpu.py holds the
conditions on the inputs: the close camera of tests/group_pack_cases.py sees only the tall box, and
every ray started on that box reaches its group, so a full wave's 64 shadow and path rays make more
than 64 items of one group -- full passes, and a remainder shared with the other groups.

Frame sizes as in tests/test_gpu_spec_groups.py: 416 x 320 x 2 SPP is the smallest frame whose waves
start with 64 pixels and reach the dual form; 48 x 40 x 4 runs the compact form (one slot)."""
import functools

import pytest

import oracle as O
import rvcp_amd
from conftest import scene_arrays
from group_pack_cases import close_camera_scene
from rvcp_amd import abi
from spec_groups import crowded_scene, three_box_scene
from test_gpu_spec_groups import _compare, _gpu

pytestmark = pytest.mark.gpu
SMALL, BIG = (48, 40, 4), (416, 320, 2)        # width, height, SPP
TIME = 123.0


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "close":
        return close_camera_scene(rvcp_amd.Scene.default())
    if name == "threebox":
        return three_box_scene()
    assert name == "crowded_close"
    return close_camera_scene(crowded_scene())


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp):
    sc = _scene(name)
    orc = O.render(scene_arrays(sc), sc.push_constant(TIME), abi.make_config(spp=spp), w, h)
    for a in orc[:2]:
        a.setflags(write=False)
    return orc


def _case(name, size, what):
    w, h, spp = size
    problems = []
    for v in (3, 6):
        got = _gpu(_scene(name), w, h, TIME, kernel_variant=v, spp=spp)
        _compare(problems, f"{what} schedule {v} {w}x{h}", got, _oracle(name, w, h, spp), v, w * h * spp)
    assert not problems, problems


def test_one_group_over_a_pass():
    """The tall box fills the frame: one group holds more than 64 items of a wave."""
    _case("close", BIG, "close camera")


def test_three_groups_dual_form():
    _case("threebox", BIG, "three boxes")


def test_three_groups_with_overflow():
    """The crowded scene under the close camera: padding before a group and a group spanning two
    passes in one wave."""
    _case("crowded_close", BIG, "crowded, close camera")


def test_compact_form():
    """The close camera at 48 x 40: the compact form (no shadow slot, one ray per lane)."""
    _case("close", SMALL, "close camera")
