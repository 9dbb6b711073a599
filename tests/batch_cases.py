"""Inputs and oracle frames for the frame-batch tests (rvcp_render_frames_async).

include/rvcp.h promises that frame k of a batch is rendered with pushes[k] -- its camera and its
time seed -- and equals rvcp_render_shard_async with the same push.  The cameras here differ in
every field a pre-pass reads (position, u / v, t_near, t_far, the field of view), so a batch
that takes any of them from another frame's record renders another picture:

    Cornell box     default       the scene's own
                    sky           the default position looking away: every pixel misses, the
                                  frame adds nothing to the batch's surface list
                    inside        within the box, t_near 0.5, t_far 2000, fov 60
                    rolled        scene.rotated_scene's camera on the unrotated mesh: no zero
                                  component, hits and misses mixed within waves
                    narrow        t_near 1, t_far 5000, fov 25
                    inside_a      on the box's axis, looking at the back wall
    sphere room     default, away, inside_glass, narrow

tests/test_batch_cases_cpu.py holds the conditions on these inputs, with the oracle alone.

Pure numpy, no GPU (test infrastructure).  Oracle frames are rendered once per distinct
(scene, config, camera, time, size) and cached; the arrays are read-only."""
import functools
import os
import re

import numpy as np

import oracle as O
import rvcp_amd
from conftest import ROOT, scene_arrays
from fuzz_scenes import _with_specks, fuzz_scene
from rvcp_amd import abi

INTERNAL_H = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc", "rvcp_internal.h")
W, H, SPP, TIME = 47, 39, 2, 3.0          # the camera tests' frame (tile_ties' size)
HYBRID_SPECKS = 160                       # test_gpu_spec_fuzz.test_bvh_hybrid_fuzz's count
FUZZ_SEEDS = (2, 3)
FUZZ_W, FUZZ_H = 48, 40

# batch order of the camera tests: the sky frame in the middle, two frames share a time
CORNELL_ORDER = ("default", "inside", "sky", "rolled", "narrow")
CORNELL_TIMES = (3.0, 7.5, 301.25, 123.0, 3.0)
SPHERE_ORDER = ("default", "away", "inside_glass", "narrow")
SPHERE_TIMES = (3.0, 7.5, 301.25, 3.0)


def _cam(pos, look, t_near, t_far, fov):
    return rvcp_amd.Camera.new(pos, look, t_near, t_far, fov, 150.0, 5.0)


@functools.lru_cache(maxsize=None)
def cornell_camera(name):
    base = rvcp_amd.Scene.default().camera
    if name == "default":
        return base
    if name == "sky":
        return _cam(base.position, base.position + np.float32([0, 0, -100]), base.t_near, base.t_far,
                    base.vertical_fov)
    if name == "inside":
        return _cam((-200, 400, -200), (200, 100, 200), 0.5, 2000.0, 60.0)
    if name == "rolled":
        return rvcp_amd.scene.rotated_scene(rvcp_amd.Scene.default()).camera
    if name == "narrow":
        return _cam(base.position, (0, 274.4, 0), 1.0, 5000.0, 25.0)
    if name == "inside_a":
        return _cam((0, 274.4, -250), (0, 274.4, 275), base.t_near, base.t_far, base.vertical_fov)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sphere_camera(name):
    if name == "default":
        return rvcp_amd.scene.sphere_scene().camera
    if name == "away":
        return _cam((0, 1, 3), (0, 1, 30), 0.1, 1000.0, 120.0)
    if name == "inside_glass":
        return _cam((1.25, 0.25, 1.25), (0, 0.5, -2), 0.01, 1000.0, 90.0)
    if name == "narrow":
        return _cam((0, 1, 3), (0, 0.3, 0), 0.5, 100.0, 40.0)
    raise KeyError(name)


def push(cam, time):
    return rvcp_amd.scene.push_constant(cam, time)


def cornell_pushes(names=CORNELL_ORDER, times=CORNELL_TIMES):
    return [push(cornell_camera(c), t) for c, t in zip(names, times)]


def sphere_pushes(names=SPHERE_ORDER, times=SPHERE_TIMES):
    return [push(sphere_camera(c), t) for c, t in zip(names, times)]


def cycled_pushes(cams, n):
    """n pushes, the cameras in turn, at times 100 + k."""
    return [push(cams[k % len(cams)], 100.0 + k) for k in range(n)]


CORNELL_CAMS = tuple(cornell_camera(c) for c in CORNELL_ORDER)
SPHERE_CAMS = tuple(sphere_camera(c) for c in SPHERE_ORDER)


# ------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def scene(name):
    """cornell (32 faces: the specialised modules exist); c6, the box with 310 small triangles
    (342 faces: the tiled schedules cross a tile, the BVH has something to hold and the hybrid
    keeps the box as its prefix); spheres, the sphere room of mode 2; fuzz<seed> and
    fuzz<seed>s, the adversarial scenes of tests/fuzz_scenes.py without and with the specks
    that make the hybrid engage."""
    if name == "cornell":
        return rvcp_amd.Scene.default()
    if name == "c6":
        return rvcp_amd.scene.with_random_triangles(rvcp_amd.Scene.default(), 310)
    if name == "spheres":
        return rvcp_amd.scene.sphere_scene()
    if name.startswith("fuzz"):
        seed = int(name[4:].rstrip("s"))
        sc = fuzz_scene(seed)[0]
        return _with_specks(sc, HYBRID_SPECKS, seed) if name.endswith("s") else sc
    raise KeyError(name)


def scene_config(name):
    """The physical configuration a scene is rendered with (the fuzz scenes come with theirs)."""
    if name.startswith("fuzz"):
        return dict(fuzz_scene(int(name[4:].rstrip("s")))[1])
    if name == "spheres":
        return dict(integrator=abi.INTEGRATOR_LEGACY, spp=SPP)
    return dict(spp=SPP)


@functools.lru_cache(maxsize=None)
def _arrays(name):
    return scene_arrays(scene(name))


# --------------------------------------------------------------------------------- threshold
def prepass_batch_max_pixels():
    """kPrepassBatchMaxPixels of csrc/rvcp_internal.h: a batch's frames of up to this many
    pixels (of this shard) share one pre-pass launch, larger ones get a launch each."""
    text = open(INTERNAL_H).read()
    m = re.search(r"constexpr\s+uint32_t\s+kPrepassBatchMaxPixels\s*=\s*([0-9uU\s*]+);", text)
    assert m, "kPrepassBatchMaxPixels not found in rvcp_internal.h"
    value = 1
    for factor in m.group(1).split("*"):
        value *= int(factor.strip().rstrip("uU"))
    return value


THRESHOLD_W = 1024


def threshold_heights():
    """(H_at, H_above): whole frames THRESHOLD_W wide with exactly P pixels and one row more."""
    p = prepass_batch_max_pixels()
    assert p % (8 * THRESHOLD_W) == 0
    return p // THRESHOLD_W, p // THRESHOLD_W + 1


def threshold_shards():
    """((H, k), (H, k)) for three shards, THRESHOLD_W wide: shard k = 2 with exactly P pixels
    while shard 0 (the slot) has one stripe more; shard k = 1 with one stripe more than P while
    the slot has two more."""
    q = prepass_batch_max_pixels() // (8 * THRESHOLD_W)      # stripes in P pixels
    return (8 * (3 * q + 1), 2), (8 * (3 * (q + 1) + 1), 1)


def t_range_ok(p, w, h):
    """rvcp_host.cpp primary_t_range_ok: t_far x t_coef stays below 2^24."""
    cam = p["camera"]
    t = np.tan(float(cam["vertical_fov"]) / 2.0 * 3.1415926 / 180.0)
    a = w / h
    return abs(float(cam["t_far"])) * np.sqrt(1.0 + t * t * (1.0 + a * a)) * (1.0 + 1e-3) < 16777216.0


# ------------------------------------------------------------------------------ oracle frames
def oracle_config(cfg):
    """rvcp_config_t of the physical fields of `cfg` alone: the schedule, the scan and the
    acceleration structure are not the oracle's business."""
    skip = ("kernel_variant", "specialize", "accel", "grid_waves_per_simd")
    return abi.make_config(**{k: v for k, v in cfg.items() if k not in skip})


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, cfg_bytes, push_bytes, w, h):
    cfg = np.frombuffer(cfg_bytes, dtype=abi.CONFIG_DTYPE)[0]
    p = np.frombuffer(push_bytes, dtype=rvcp_amd.scene.PUSH_DTYPE)[0]
    lin, rgba, trav = O.render(_arrays(name), p, cfg, w, h)
    lin.setflags(write=False)
    rgba.setflags(write=False)
    return lin, rgba, trav


def oracle_frames(name, cfg, pushes, w, h, k=0, n=1):
    """[(linear, rgba, traversals)] of shard k of n of every push's frame: the oracle's whole
    frame (rendered once per camera, time and size) cut to the shard's rows, the traversals
    those of the shard's pixels (a second render of the rows when the shard is not the frame)."""
    ocfg = oracle_config(cfg)
    rows = rvcp_amd.shard_row_ids(h, k, n)
    out = []
    for p in pushes:
        p = np.ascontiguousarray(p, dtype=rvcp_amd.scene.PUSH_DTYPE)
        lin, rgba, trav = _oracle_frame(name, ocfg.tobytes(), p.tobytes(), w, h)
        if n > 1:
            trav = _shard_traversals(name, ocfg.tobytes(), p.tobytes(), w, h, k, n)
            lin, rgba = lin[rows], rgba[rows]
        out.append((lin, rgba, trav))
    return out


@functools.lru_cache(maxsize=None)
def _shard_traversals(name, cfg_bytes, push_bytes, w, h, k, n):
    """The oracle's traversal count over the rows of shard k of n: its stripes rendered one
    rectangle each (the count of a rectangle is the sum over its pixels)."""
    cfg = np.frombuffer(cfg_bytes, dtype=abi.CONFIG_DTYPE)[0]
    p = np.frombuffer(push_bytes, dtype=rvcp_amd.scene.PUSH_DTYPE)[0]
    whole = _oracle_frame(name, cfg_bytes, push_bytes, w, h)
    total = 0
    for s in range(k, (h + 7) // 8, n):
        y0, th = 8 * s, min(8, h - 8 * s)
        lin, _, trav = O.render(_arrays(name), p, cfg, w, h, rect=(0, y0, w, th))
        assert np.array_equal(lin.view(np.uint32), whole[0][y0:y0 + th].view(np.uint32))
        total += trav
    return total
