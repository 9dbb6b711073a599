"""Shared by tests/test_group_pack_cpu.py and tests/test_gpu_group_pack.py (DESIGN.md §4.7 "Face
groups", the item layout of csrc/rvcp_group_pack.h): the close camera that makes one group hold
more items than a pass, and the CPU build of a scene's reach test.  Pure test infrastructure.

The tall box of the Cornell box (faces 12..21, group 0) stands on x in [-10, 197], z in [-28, 181],
330 high; its side towards the camera runs from (148, -28) to (-10, 21).  The close camera stands
100 in front of the middle of that side at half the box's height and looks at it: with the 40
degree vertical field of view the frame spans 73 x 95 of a 330 x 165 face, so every primary ray
of a 416 x 320 frame lands on it and every first shadow and path ray of a wave starts on the
tall box.  (The crowded scene widens that box by 1.08 about its centre: the side moves 7 closer.)"""
import ctypes
import subprocess

import numpy as np

import rvcp_amd
from spec_groups import GROUP_PRELUDE, GroupedScan
from test_jit_cpu import PRELUDE, _scan_source

TALL_BOX_FACES = tuple(range(12, 22))
CLOSE_POSITION = (39.4, 165.0, -99.0)
CLOSE_LOOK_AT = (69.0, 165.0, -3.5)


def close_camera_scene(base):
    """`base` (the Cornell box or a scene built on it) seen by the close camera."""
    cam = base.camera
    camera = rvcp_amd.scene.Camera.new(CLOSE_POSITION, CLOSE_LOOK_AT, cam.t_near, cam.t_far,
                                       cam.vertical_fov, cam.move_speed, cam.rotate_speed)
    return rvcp_amd.Scene(camera, list(base.materials), list(base.spheres), base.mesh)


REACH_DRIVER = r"""
// mask[r]: the groups ray r reaches over [tmin, bound] (spec_group_reach), or -1 for a ray the
// grouped scan's guard turns away
extern "C" void reach_all(const float *rays, int n, float tmin, float bound, int rcp_mode, int *mask) {
    g_rcp_mode = rcp_mode;
    for (int r = 0; r < n; r++) {
        const float *q = rays + 6 * r;
        const f3 o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
        mask[r] = spec_group_origin_ok(o) ? (int)spec_group_reach(o, d, tmin, bound) : -1;
    }
}
"""


def reach_masks(tmp_path, gs: GroupedScan, name, rays, tmin, bound, rcp_mode=0):
    """The reach test of `gs`'s generated text for every ray: [R] int32 group masks."""
    src = tmp_path / f"{name}_reach.cpp"
    src.write_text(PRELUDE + GROUP_PRELUDE + _scan_source(gs.rec) + gs.text + REACH_DRIVER)
    so = tmp_path / f"{name}_reach.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma",
                    "-fno-fast-math", "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.reach_all.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                              ctypes.c_void_p]
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    mask = np.zeros(len(rays), np.int32)
    lib.reach_all(rays.ctypes.data, len(rays), tmin, bound, rcp_mode, mask.ctypes.data)
    return mask
