"""The schedule a real render reports against the frame plan's reference.

csrc/rvcp_frame_plan.cpp decides a render's schedule and specialised kernels;
tests/test_frame_plan_cpu.py holds it against tests/frame_plan_ref.py on the CPU.  Here the
library renders and rvcp_stats_t.kernel_variant must be the reference's stats code: on the small
frame, on either side of kTiledDualMinSamples (10 vs 5 on a 342-face mesh) and of
kWideMinSamples (6 vs 3 with the generic scan), under the BVH with and without the hybrid's
module, in mode 2, for a black frame, and for a 3-frame batch of every route (refused ones
included).  No pixels are compared: the oracle suites hold those."""
import pytest

import batch_cases as B
import frame_plan_ref as R
import rvcp_amd
from rvcp_amd import abi

OFF = abi.SPECIALIZE_OFF
BVH = abi.ACCEL_BVH
LEGACY = abi.INTEGRATOR_LEGACY
K = R.constants()


def _module(cfg, scene_name):
    """(the specialised module upload builds for the scene, the hybrid's prefix): the Cornell
    box and the sphere room are within the JIT's 64 faces; c6 is not, but the hybrid keeps the
    box, its first 32 faces, out of the BVH and scans them with a module."""
    if cfg.get("specialize", abi.SPECIALIZE_AUTO) == OFF:
        return "absent", 0
    if cfg.get("accel", abi.ACCEL_NONE) == BVH:
        return ("complete", 32) if scene_name == "c6" else ("absent", 0)
    return ("complete" if scene_name in ("cornell", "spheres") else "absent"), 0


def _reference(cfg, scene_name, w, h, n_frames=1):
    c = abi.make_config(**cfg)
    module, prefix = _module(cfg, scene_name)
    inp = R.make_input(module, bvh_prefix=prefix, n_frames=n_frames, frame_px=w * h, stride=w * h,
                       n_faces=len(B.scene(scene_name).mesh.aligned_faces()),
                       **{k: c[k].item() for k in ("integrator", "kernel_variant", "accel", "spp",
                                                   "max_bounces", "attenuation_stop_eps",
                                                   "ray_t_min", "grid_waves_per_simd")})
    return R.plan(inp)


def _tracer(cfg, scene_name):
    rt = rvcp_amd.RayTracer(**cfg)
    rt.upload_scene(B.scene(scene_name))
    return rt


def _single(cfg, scene_name, w, h):
    """(kernel_variant of one rendered frame, the reference's plan)"""
    with _tracer(cfg, scene_name) as rt:
        rt.render(w, h, B.TIME)
        return int(rt.last_stats["kernel_variant"]), _reference(cfg, scene_name, w, h)


SMALL = dict(spp=B.SPP)
SINGLE_CASES = {
    # name: (scene, config, W, H, the code the issue names)
    "cornell_auto": ("cornell", SMALL, B.W, B.H, 3 | abi.VARIANT_SPECIALIZED),
    "cornell_off": ("cornell", dict(SMALL, specialize=OFF), B.W, B.H, 3),
    "c6_small": ("c6", SMALL, B.W, B.H, 5),
    "c6_at_dual": ("c6", dict(spp=8), 256, 256, 10),
    "c6_below_dual": ("c6", dict(spp=7), 256, 256, 5),
    "cornell_off_at_wide": ("cornell", dict(spp=32, specialize=OFF), 512, 512, 6),
    "cornell_off_below_wide": ("cornell", dict(spp=31, specialize=OFF), 512, 512, 3),
    "bvh": ("c6", dict(SMALL, accel=BVH, specialize=OFF), B.W, B.H, 7),
    "bvh_hybrid": ("c6", dict(SMALL, accel=BVH), B.W, B.H, 7 | abi.VARIANT_SPECIALIZED),
    "mode2": ("spheres", dict(SMALL, integrator=LEGACY, specialize=OFF), B.W, B.H, 8),
    "mode2_spec": ("spheres", dict(SMALL, integrator=LEGACY), B.W, B.H, 8 | abi.VARIANT_SPECIALIZED),
    "no_bounces": ("cornell", dict(SMALL, max_bounces=0), B.W, B.H, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE_CASES)
def test_single_frame_schedule(name):
    scene_name, cfg, w, h, code = SINGLE_CASES[name]
    got, ref = _single(cfg, scene_name, w, h)
    assert ref["status"] == abi.RVCP_OK and ref["stats_code"] == code      # the case is what it says
    assert got == ref["stats_code"]


def test_threshold_cases_sit_at_the_thresholds():
    assert 256 * 256 * 8 == K["kTiledDualMinSamples"] and 512 * 512 * 32 == K["kWideMinSamples"]
    assert 342 >= K["kTiledMinFaces"] and 32 <= K["kTiledWideMinFaces"]


# a 3-frame batch of every route at 47 x 39: route -> (scene, config)
BATCH_ROUTES = {
    "r1": ("cornell", dict(kernel_variant=1)), "r2": ("cornell", dict(kernel_variant=2)),
    "r3g": ("cornell", dict(kernel_variant=3, specialize=OFF)), "r3s": ("cornell", dict(kernel_variant=3)),
    "r6g": ("cornell", dict(kernel_variant=6, specialize=OFF)), "r6s": ("cornell", dict(kernel_variant=6)),
    "r4": ("c6", dict(kernel_variant=4)), "r5": ("c6", dict(kernel_variant=5)),
    "r10": ("c6", dict(kernel_variant=10)), "auto": ("cornell", dict()), "auto_c6": ("c6", dict()),
    "bvh": ("c6", dict(accel=BVH, specialize=OFF)), "hybrid": ("c6", dict(accel=BVH)),
    "m2g": ("spheres", dict(integrator=LEGACY, specialize=OFF)), "m2s": ("spheres", dict(integrator=LEGACY)),
    "r1_black": ("cornell", dict(kernel_variant=1, max_bounces=0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("route", BATCH_ROUTES)
def test_batch_schedule(route):
    import torch
    scene_name, cfg = BATCH_ROUTES[route]
    cfg = dict(SMALL, **cfg)
    sc = B.scene(scene_name)
    pushes = [sc.push_constant(B.TIME + k) for k in range(3)]
    ref = _reference(cfg, scene_name, B.W, B.H, n_frames=3)
    assert (ref["status"] != abi.RVCP_OK) == (route in ("r1", "r2"))
    out = torch.zeros((3 * B.W * B.H,), dtype=torch.int32, device="cuda")
    with _tracer(cfg, scene_name) as rt:
        if ref["status"] != abi.RVCP_OK:
            with pytest.raises(abi.RvcpError) as e:
                rt.render_frames_async(pushes, B.W, B.H, 0, 1, out.data_ptr())
            assert e.value.code == ref["status"] == abi.RVCP_E_UNSUPPORTED
            return
        rt.render_frames_async(pushes, B.W, B.H, 0, 1, out.data_ptr())
        st = rt.sync_stats().copy()
        torch.cuda.synchronize()
    assert int(st["kernel_variant"]) == ref["stats_code"]
    assert int(st["samples"]) == 3 * B.W * B.H * cfg["spp"]
