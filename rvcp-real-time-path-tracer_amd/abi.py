"""ctypes binding of librvcp (include/rvcp.h) -- the product's C-ABI.

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950)
into ``csrc/build/librvcp.so``.  There is no fallback: if the library is missing,
``load()`` raises, so nothing can silently run a CPU path in its place.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVCP_LIB") or os.path.join(_HERE, "csrc", "build", "librvcp.so")

# rvcp_config_t (include/rvcp.h)
CONFIG_DTYPE = np.dtype([("device", "<i4"), ("integrator", "<i4"), ("spp", "<u4"),
                         ("max_bounces", "<u4"), ("attenuation_stop_eps", "<f4"),
                         ("ray_t_min", "<f4"), ("ray_t_max", "<f4"), ("rr_probability", "<f4"),
                         ("eps", "<f4"), ("lum_id_std140_quirk", "<i4"), ("kernel_variant", "<i4"),
                         ("accel", "<i4"), ("n_gpus", "<i4"), ("unorm_rule", "<i4"),
                         ("specialize", "<i4"), ("grid_waves_per_simd", "<u4")])
STATS_DTYPE = np.dtype([("kernel_ms", "<f8"), ("traversals", "<u8"),
                        ("traversals_executed", "<u8"), ("samples", "<u8"), ("faces", "<u4"),
                        ("kernel_variant", "<i4"), ("wave_iterations", "<u8"),
                        ("main_kernel_ms", "<f8"), ("shader_clock_ghz", "<f8")])
assert CONFIG_DTYPE.itemsize == 64 and STATS_DTYPE.itemsize == 64
# rvcp_gbuffer_texel_t / rvcp_denoise_params_t (G-buffer and a-trous denoiser)
GBUFFER_DTYPE = np.dtype([("position", "<f4", (3,)), ("face", "<u4"),
                          ("normal", "<f4", (3,)), ("material", "<u4")])
DENOISE_PARAMS_DTYPE = np.dtype([("iterations", "<u4"), ("normal_power_log2", "<u4"),
                                 ("sigma_color", "<f4"), ("sigma_plane", "<f4")])
assert GBUFFER_DTYPE.itemsize == 32 and DENOISE_PARAMS_DTYPE.itemsize == 16
GBUFFER_MISS, GBUFFER_EMISSIVE = 0xFFFFFFFF, 0x80000000
DENOISE_MAX_ITERATIONS = 8
# rvcp_temporal_params_t / rvcp_temporal_view_t (temporal accumulation)
TEMPORAL_PARAMS_DTYPE = np.dtype([("alpha_min", "<f4"), ("max_history", "<u4"),
                                  ("sigma_plane", "<f4"), ("normal_min", "<f4")])
TEMPORAL_VIEW_DTYPE = np.dtype([("position", "<f4", (3,)), ("k", "<f4"),
                                ("right", "<f4", (3,)), ("_pad0", "<f4"),
                                ("down", "<f4", (3,)), ("_pad1", "<f4"),
                                ("forward", "<f4", (3,)), ("_pad2", "<f4")])
assert TEMPORAL_PARAMS_DTYPE.itemsize == 16 and TEMPORAL_VIEW_DTYPE.itemsize == 64
TEMPORAL_MAX_HISTORY = 65535
TEMPORAL_DENOISE = 1            # rvcp_render_temporal flags
# rvcp_svgf_params_t (moments, variance and the variance-guided filter)
SVGF_PARAMS_DTYPE = np.dtype([("iterations", "<u4"), ("normal_power_log2", "<u4"),
                              ("sigma_luminance", "<f4"), ("sigma_plane", "<f4"),
                              ("epsilon", "<f4"), ("alpha_moments_min", "<f4"),
                              ("spatial_below", "<u4"), ("_pad", "<u4")])
assert SVGF_PARAMS_DTYPE.itemsize == 32
SVGF_MAX_ITERATIONS, SVGF_MAX_SPATIAL_BELOW = 8, 16
SVGF_FEEDBACK = 1               # rvcp_render_svgf flags
# rvcp_taa_params_t (temporal anti-aliasing: jitter and the clamped resolve)
TAA_PARAMS_DTYPE = np.dtype([("alpha_min", "<f4"), ("max_history", "<u4"), ("clamp", "<u4"),
                             ("_pad", "<u4")])
assert TAA_PARAMS_DTYPE.itemsize == 16
TAA_JITTER_PERIOD = 16
# rvcp_taau_params_t (temporal upsampling)
TAAU_PARAMS_DTYPE = np.dtype([("max_weight", "<f4"), ("init_weight", "<f4"), ("clamp", "<u4"),
                              ("_pad", "<u4")])
assert TAAU_PARAMS_DTYPE.itemsize == 16
# rvcp_adaptive_params_t (adaptive sampling: the plan step and the switch)
ADAPTIVE_PARAMS_DTYPE = np.dtype([("spp_min", "<u4"), ("spp_max", "<u4"), ("mean_spp", "<f4"),
                                  ("weight_cap", "<f4"), ("epsilon", "<f4"), ("_pad", "<u4")])
assert ADAPTIVE_PARAMS_DTYPE.itemsize == 24
SPP_MAP_MAX = 256               # RVCP_SPP_MAP_MAX
# rvcp_ray_t / rvcp_ray_hit_t (ray queries)
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("d", "<f4", (3,)), ("t_min", "<f4"), ("t_max", "<f4")])
RAY_HIT_DTYPE = np.dtype([("face", "<i4"), ("t", "<f4"), ("b1", "<f4"), ("b2", "<f4")])
assert RAY_DTYPE.itemsize == 32 and RAY_HIT_DTYPE.itemsize == 16
RAYS_NEAREST, RAYS_ANY = 0, 1
# rvcp_stats_t.kernel_variant -> the dominant kernel's name as rocprofv3 reports it
KERNEL_NAMES = {1: "games101_kernel", 2: "games101_dual_kernel", 3: "games101_path_kernel<5>",
                4: "games101_tiled_kernel", 5: "games101_tiled_single_kernel",
                6: "games101_path_kernel<6>", 7: "games101_bvh_path_kernel", 8: "legacy_kernel",
                10: "games101_tiled_pool_kernel", 11: "path_scatter_kernel",
                # + RVCP_VARIANT_SPECIALIZED (16): the scene-specialised module (rvcp_jit.cpp)
                19: "rvcp_spec_path_kernel5", 22: "rvcp_spec_path_kernel6", 23: "rvcp_spec_bvh_path_kernel",
                24: "rvcp_spec_legacy_kernel"}
VARIANT_SPECIALIZED = 16

# Defaults == the shader's #defines (ray_tracer_games101_branch.comp:5-13).
DEFAULTS = dict(device=0, integrator=0, spp=20, max_bounces=15, attenuation_stop_eps=0.05,
                ray_t_min=0.01, ray_t_max=10000.0, rr_probability=0.8, eps=0.001,
                lum_id_std140_quirk=1, kernel_variant=0, accel=0, n_gpus=1, unorm_rule=0, specialize=0,
                grid_waves_per_simd=0)

# Error codes
RVCP_OK, RVCP_E_INVALID, RVCP_E_HIP, RVCP_E_NO_SCENE, RVCP_E_UNSUPPORTED, RVCP_E_NOMEM, \
    RVCP_E_INTERNAL, RVCP_E_TIMEOUT, RVCP_E_BUSY = 0, -1, -2, -3, -4, -5, -6, -7, -8
# RVCP_ABI_VERSION of include/rvcp.h this binding's struct layouts follow (load() checks it)
ABI_VERSION = 2
RCCL_ID_BYTES = 128

EXPORTED = ["rvcp_version", "rvcp_config_default", "rvcp_config_default_for", "rvcp_create",
            "rvcp_destroy", "rvcp_last_error", "rvcp_upload_scene", "rvcp_render", "rvcp_render_shard_async",
            "rvcp_sync_stats", "rvcp_shard_rows", "rvcp_assemble_frame_async",
            "rvcp_upload_scene_file", "rvcp_mandelbrot", "rvcp_render_async", "rvcp_wait",
            "rvcp_rccl_unique_id", "rvcp_rccl_init", "rvcp_rccl_attach", "rvcp_gather_frame_async",
            "rvcp_gather_wait", "rvcp_render_frames_async", "rvcp_rccl_set_timeout",
            "rvcp_abi_version", "rvcp_set_code_cache_dir", "rvcp_code_cache_counts",
            "rvcp_render_gbuffer_async", "rvcp_denoise_params_default", "rvcp_denoise_async",
            "rvcp_denoise_wait", "rvcp_render_denoised",
            "rvcp_temporal_params_default", "rvcp_temporal_view_from_push",
            "rvcp_temporal_accumulate_async", "rvcp_temporal_wait", "rvcp_render_temporal",
            "rvcp_temporal_reset",
            "rvcp_svgf_params_default", "rvcp_svgf_accumulate_async", "rvcp_svgf_filter_async",
            "rvcp_svgf_wait", "rvcp_render_svgf", "rvcp_svgf_reset",
            "rvcp_demodulate_async", "rvcp_remodulate_async", "rvcp_albedo_wait",
            "rvcp_set_demodulation", "rvcp_get_demodulation",
            "rvcp_taa_jitter", "rvcp_taa_jitter_push", "rvcp_taa_params_default",
            "rvcp_taa_resolve_async", "rvcp_taa_wait", "rvcp_set_taa", "rvcp_get_taa",
            "rvcp_taa_reset",
            "rvcp_taau_params_default", "rvcp_taa_upsample_async", "rvcp_taau_wait",
            "rvcp_set_taa_upsample", "rvcp_get_taa_upsample",
            "rvcp_set_sampling", "rvcp_get_sampling", "rvcp_set_materials", "rvcp_get_materials",
            "rvcp_render_spp_map_async", "rvcp_adaptive_params_default", "rvcp_spp_plan_async",
            "rvcp_spp_plan_wait", "rvcp_set_adaptive", "rvcp_get_adaptive",
            "rvcp_adaptive_last_map",
            "rvcp_trace_rays_async", "rvcp_rays_wait", "rvcp_trace_rays", "rvcp_primary_rays_async",
            "rvcp_pick",
            "rvcp_trace_paths_async", "rvcp_paths_wait", "rvcp_trace_paths",
            "rvcp_primary_seeds_async"]


# Integrator mode 2 (ray_tracer.comp ray_trace): its own #defines (ray_tracer.comp:5-13).
LEGACY_DEFAULTS = dict(device=0, integrator=1, spp=5, max_bounces=3, attenuation_stop_eps=0.01,
                       ray_t_min=0.01, ray_t_max=1000.0, rr_probability=1.0, eps=0.001,
                       lum_id_std140_quirk=1, kernel_variant=0, accel=0, n_gpus=1, unorm_rule=0, specialize=0,
                       grid_waves_per_simd=0)
INTEGRATOR_GAMES101, INTEGRATOR_LEGACY = 0, 1
ACCEL_NONE, ACCEL_BVH = 0, 1
UNORM_DRIVER, UNORM_NEAREST = 0, 1
SPECIALIZE_AUTO, SPECIALIZE_OFF = 0, 1
# rvcp_set_sampling: the games101 bounce
SAMPLING_UNIFORM, SAMPLING_COSINE = 0, 1
# rvcp_set_materials: material scattering on meshes
MATERIALS_LAMBERTIAN, MATERIALS_SCATTER = 0, 1


def make_config(**kw) -> np.ndarray:
    """rvcp_config_t with the #define defaults of the selected integrator, overridden by kw."""
    cfg = np.zeros((), dtype=CONFIG_DTYPE)
    vals = dict(LEGACY_DEFAULTS if kw.get("integrator", 0) == INTEGRATOR_LEGACY else DEFAULTS)
    vals.update(kw)
    for k, v in vals.items():
        cfg[k] = v
    return cfg


def make_denoise_params(**overrides) -> np.ndarray:
    """rvcp_denoise_params_t with the library's defaults (rvcp_denoise_params_default),
    overridden by the keyword arguments (sigma_color=float("inf") switches the colour weight
    off)."""
    p = np.zeros((), dtype=DENOISE_PARAMS_DTYPE)
    rc = load().rvcp_denoise_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_denoise_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def make_temporal_params(**overrides) -> np.ndarray:
    """rvcp_temporal_params_t with the library's defaults (rvcp_temporal_params_default),
    overridden by the keyword arguments."""
    p = np.zeros((), dtype=TEMPORAL_PARAMS_DTYPE)
    rc = load().rvcp_temporal_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_temporal_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def make_svgf_params(**overrides) -> np.ndarray:
    """rvcp_svgf_params_t with the library's defaults (rvcp_svgf_params_default), overridden by
    the keyword arguments (sigma_luminance=float("inf") switches the luminance weight off)."""
    p = np.zeros((), dtype=SVGF_PARAMS_DTYPE)
    rc = load().rvcp_svgf_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_svgf_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def make_taa_params(**overrides) -> np.ndarray:
    """rvcp_taa_params_t with the library's defaults (rvcp_taa_params_default), overridden by the
    keyword arguments."""
    p = np.zeros((), dtype=TAA_PARAMS_DTYPE)
    rc = load().rvcp_taa_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_taa_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def make_taau_params(**overrides) -> np.ndarray:
    """rvcp_taau_params_t with the library's defaults (rvcp_taau_params_default), overridden by
    the keyword arguments."""
    p = np.zeros((), dtype=TAAU_PARAMS_DTYPE)
    rc = load().rvcp_taau_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_taau_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def make_adaptive_params(**overrides) -> np.ndarray:
    """rvcp_adaptive_params_t with the library's defaults (rvcp_adaptive_params_default),
    overridden by the keyword arguments."""
    p = np.zeros((), dtype=ADAPTIVE_PARAMS_DTYPE)
    rc = load().rvcp_adaptive_params_default(ptr(p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_adaptive_params_default failed")
    for k, v in overrides.items():
        p[k] = v
    return p


def taa_jitter(frame_index: int) -> np.ndarray:
    """rvcp_taa_jitter: the sub-pixel jitter (jx, jy) of frame `frame_index`, in pixels: the
    Halton(2, 3) point of index frame_index % TAA_JITTER_PERIOD + 1, centred."""
    j = np.zeros(2, dtype=np.float32)
    rc = load().rvcp_taa_jitter(int(frame_index) & 0xFFFFFFFF, ptr(j))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_taa_jitter failed")
    return j


def taa_jitter_push(push, width: int, height: int, jitter) -> np.ndarray:
    """rvcp_taa_jitter_push: a copy of `push` whose camera looks `jitter` pixels off (forward
    rotated towards right / down, its length kept); a zero jitter returns the same bytes."""
    from .scene import PUSH_DTYPE
    push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
    j = np.ascontiguousarray(jitter, dtype=np.float32).reshape(2)
    out = np.zeros_like(push)
    rc = load().rvcp_taa_jitter_push(ptr(push), width, height, ptr(j), ptr(out))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_taa_jitter_push failed")
    return out


def temporal_view(push, width: int, height: int) -> np.ndarray:
    """rvcp_temporal_view_from_push: the camera of a push constant as rvcp_temporal_view_t, the
    `view` of the NEXT frame's rvcp_temporal_accumulate_async."""
    from .scene import PUSH_DTYPE
    push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
    v = np.zeros((), dtype=TEMPORAL_VIEW_DTYPE)
    rc = load().rvcp_temporal_view_from_push(ptr(push), width, height, ptr(v))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_temporal_view_from_push failed")
    return v


class RvcpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rvcp error {code}: {msg}")
        self.code = code


_lib = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm bundles its own libamdhip64.so and NEEDs it by the unversioned name, while
    librvcp NEEDs libamdhip64.so.7.  If librvcp loaded first, a later `import torch` would
    load a SECOND HIP runtime that sees no GPU.  Preloading torch's copy (soname
    libamdhip64.so.7) makes both resolve to one runtime whatever the import order, so device
    pointers and streams from torch are valid in librvcp.  RVCP_HIP_RUNTIME=system skips it."""
    if os.environ.get("RVCP_HIP_RUNTIME") == "system":
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    # (RCCL is not preloaded: librvcp dlopen()s "librccl.so.1" when a gather needs it, which
    # resolves by soname to the copy `import torch` already loaded.  Preloading torch's
    # librccl.so before torch itself aborts the interpreter at exit.)
    for d in spec.submodule_search_locations:
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            f = os.path.join(d, "lib", name)
            if os.path.exists(f):
                ctypes.CDLL(f, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load librvcp.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"librvcp.so not built ({LIB_PATH}); run __graft_entry__.build()")
    _share_torch_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.rvcp_version.restype = ctypes.c_char_p
    L.rvcp_abi_version.restype = u32
    L.rvcp_set_code_cache_dir.argtypes = [ctypes.c_char_p]
    L.rvcp_code_cache_counts.argtypes = [P]
    L.rvcp_config_default.argtypes = [P]
    L.rvcp_config_default_for.argtypes = [ctypes.c_int32, P]
    L.rvcp_create.argtypes = [P, ctypes.POINTER(ctypes.c_void_p)]
    L.rvcp_destroy.argtypes = [P]
    L.rvcp_last_error.argtypes = [P]
    L.rvcp_last_error.restype = ctypes.c_char_p
    L.rvcp_upload_scene.argtypes = [P, P, u32, P, u32, P, u32, P, u32, P, u32, P, u32]
    L.rvcp_upload_scene_file.argtypes = [P, ctypes.c_char_p, P]
    L.rvcp_mandelbrot.argtypes = [P, P, u32, u32, P, P, P]
    L.rvcp_render.argtypes = [P, P, u32, u32, P, P, P]
    L.rvcp_render_shard_async.argtypes = [P, P, u32, u32, u32, u32, P, P, P]
    L.rvcp_render_frames_async.argtypes = [P, P, u32, u32, u32, u32, u32, P, P, P]
    L.rvcp_sync_stats.argtypes = [P, P]
    L.rvcp_render_async.argtypes = [P, P, u32, u32, P, P, P]
    L.rvcp_wait.argtypes = [P, P]
    L.rvcp_shard_rows.argtypes = [u32, u32, u32]
    L.rvcp_shard_rows.restype = u32
    L.rvcp_assemble_frame_async.argtypes = [P, P, u32, u32, u32, u32, P, P]
    L.rvcp_rccl_unique_id.argtypes = [P]
    L.rvcp_rccl_init.argtypes = [P, P, u32, u32]
    L.rvcp_rccl_attach.argtypes = [P, P, u32, u32]
    L.rvcp_rccl_set_timeout.argtypes = [P, u32]
    L.rvcp_gather_frame_async.argtypes = [P, P, u32, u32, P, P, P]
    L.rvcp_gather_wait.argtypes = [P, P, P]
    L.rvcp_render_gbuffer_async.argtypes = [P, P, u32, u32, P, P]
    L.rvcp_denoise_params_default.argtypes = [P]
    L.rvcp_denoise_async.argtypes = [P, P, P, u32, u32, P, P, P, P]
    L.rvcp_denoise_wait.argtypes = [P, P]
    L.rvcp_render_denoised.argtypes = [P, P, u32, u32, P, P, P, P, P]
    L.rvcp_temporal_params_default.argtypes = [P]
    L.rvcp_temporal_view_from_push.argtypes = [P, u32, u32, P]
    L.rvcp_temporal_accumulate_async.argtypes = [P, P, P, P, P, P, P, u32, u32, P, P, P, P, P]
    L.rvcp_temporal_wait.argtypes = [P, P]
    L.rvcp_render_temporal.argtypes = [P, P, u32, u32, P, u32, P, P, P, P, P, P, P]
    L.rvcp_temporal_reset.argtypes = [P]
    L.rvcp_svgf_params_default.argtypes = [P]
    L.rvcp_svgf_accumulate_async.argtypes = [P, P, P, P, P, P, P, P, u32, u32, P, P, P, P, P, P, P]
    L.rvcp_svgf_filter_async.argtypes = [P, P, P, P, P, u32, u32, P, P, P, P, P, P]
    L.rvcp_svgf_wait.argtypes = [P, P, P]
    L.rvcp_render_svgf.argtypes = [P, P, u32, u32, P, P, u32, P, P, P, P, P, P, P]
    L.rvcp_svgf_reset.argtypes = [P]
    L.rvcp_demodulate_async.argtypes = [P, P, P, u32, u32, P, P]
    L.rvcp_remodulate_async.argtypes = [P, P, P, u32, u32, P, P, P]
    L.rvcp_albedo_wait.argtypes = [P, P, P]
    L.rvcp_set_demodulation.argtypes = [P, ctypes.c_int]
    L.rvcp_get_demodulation.argtypes = [P, P]
    L.rvcp_taa_jitter.argtypes = [u32, P]
    L.rvcp_taa_jitter_push.argtypes = [P, u32, u32, P, P]
    L.rvcp_taa_params_default.argtypes = [P]
    L.rvcp_taa_resolve_async.argtypes = [P, P, P, P, P, P, P, u32, u32, P, P, P, P, P]
    L.rvcp_taa_wait.argtypes = [P, P]
    L.rvcp_set_taa.argtypes = [P, ctypes.c_int]
    L.rvcp_get_taa.argtypes = [P, P]
    L.rvcp_taa_reset.argtypes = [P]
    L.rvcp_taau_params_default.argtypes = [P]
    L.rvcp_taa_upsample_async.argtypes = [P, u32, P, P, P, P, P, P, P, u32, u32, P, P, P, P, P]
    L.rvcp_taau_wait.argtypes = [P, P]
    L.rvcp_set_taa_upsample.argtypes = [P, u32]
    L.rvcp_get_taa_upsample.argtypes = [P, P]
    L.rvcp_set_sampling.argtypes = [P, ctypes.c_int32]
    L.rvcp_get_sampling.argtypes = [P, P]
    L.rvcp_set_materials.argtypes = [P, ctypes.c_int32]
    L.rvcp_get_materials.argtypes = [P, P]
    L.rvcp_render_spp_map_async.argtypes = [P, P, u32, u32, P, u32, P, P, P]
    L.rvcp_adaptive_params_default.argtypes = [P]
    L.rvcp_spp_plan_async.argtypes = [P, P, P, P, P, u32, u32, P, P, P]
    L.rvcp_spp_plan_wait.argtypes = [P, P, P]
    L.rvcp_set_adaptive.argtypes = [P, P]
    L.rvcp_get_adaptive.argtypes = [P, P, P]
    L.rvcp_adaptive_last_map.argtypes = [P, P, P, P]
    L.rvcp_trace_rays_async.argtypes = [P, P, u32, u32, P, P]
    L.rvcp_rays_wait.argtypes = [P, P]
    L.rvcp_trace_rays.argtypes = [P, P, u32, u32, P, P]
    L.rvcp_primary_rays_async.argtypes = [P, P, u32, u32, P, P]
    L.rvcp_pick.argtypes = [P, P, u32, u32, u32, u32, P]
    L.rvcp_trace_paths_async.argtypes = [P, P, P, u32, u32, P, P]
    L.rvcp_paths_wait.argtypes = [P, P, P]
    L.rvcp_trace_paths.argtypes = [P, P, P, u32, u32, P, P, P]
    L.rvcp_primary_seeds_async.argtypes = [P, P, u32, u32, P, P]
    for name in ("rvcp_config_default", "rvcp_config_default_for", "rvcp_create", "rvcp_destroy", "rvcp_upload_scene",
                 "rvcp_render", "rvcp_render_shard_async", "rvcp_sync_stats",
                 "rvcp_assemble_frame_async", "rvcp_upload_scene_file", "rvcp_mandelbrot",
                 "rvcp_render_async", "rvcp_wait", "rvcp_rccl_unique_id", "rvcp_rccl_init",
                 "rvcp_rccl_attach", "rvcp_gather_frame_async", "rvcp_gather_wait",
                 "rvcp_render_frames_async", "rvcp_rccl_set_timeout", "rvcp_set_code_cache_dir",
                 "rvcp_code_cache_counts", "rvcp_render_gbuffer_async",
                 "rvcp_denoise_params_default", "rvcp_denoise_async", "rvcp_denoise_wait",
                 "rvcp_render_denoised", "rvcp_temporal_params_default",
                 "rvcp_temporal_view_from_push", "rvcp_temporal_accumulate_async",
                 "rvcp_temporal_wait", "rvcp_render_temporal", "rvcp_temporal_reset",
                 "rvcp_svgf_params_default", "rvcp_svgf_accumulate_async",
                 "rvcp_svgf_filter_async", "rvcp_svgf_wait", "rvcp_render_svgf",
                 "rvcp_svgf_reset", "rvcp_demodulate_async", "rvcp_remodulate_async",
                 "rvcp_albedo_wait", "rvcp_set_demodulation", "rvcp_get_demodulation",
                 "rvcp_taa_jitter", "rvcp_taa_jitter_push", "rvcp_taa_params_default",
                 "rvcp_taa_resolve_async", "rvcp_taa_wait", "rvcp_set_taa", "rvcp_get_taa",
                 "rvcp_taa_reset", "rvcp_taau_params_default", "rvcp_taa_upsample_async",
                 "rvcp_taau_wait", "rvcp_set_taa_upsample", "rvcp_get_taa_upsample",
                 "rvcp_set_sampling", "rvcp_get_sampling", "rvcp_set_materials",
                 "rvcp_get_materials", "rvcp_render_spp_map_async",
                 "rvcp_adaptive_params_default", "rvcp_spp_plan_async", "rvcp_spp_plan_wait",
                 "rvcp_set_adaptive", "rvcp_get_adaptive", "rvcp_adaptive_last_map",
                 "rvcp_trace_rays_async", "rvcp_rays_wait", "rvcp_trace_rays",
                 "rvcp_primary_rays_async", "rvcp_pick",
                 "rvcp_trace_paths_async", "rvcp_paths_wait", "rvcp_trace_paths",
                 "rvcp_primary_seeds_async"):
        getattr(L, name).restype = ctypes.c_int
    if L.rvcp_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI revision {L.rvcp_abi_version()}, this binding "
                           f"follows {ABI_VERSION} (rebuild: __graft_entry__.build())")
    _lib = L
    return L


def ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def set_code_cache_dir(path):
    """rvcp_set_code_cache_dir: the on-disk cache of scene-specialised code objects (None or ""
    disables it; default $XDG_CACHE_HOME/rvcp-mi355x, else ~/.cache/rvcp-mi355x)."""
    rc = load().rvcp_set_code_cache_dir(None if path is None else os.fsencode(path))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_set_code_cache_dir failed")


def code_cache_counts():
    """rvcp_code_cache_counts: dict(loads, compiles, rejects) of the on-disk module cache."""
    out = (ctypes.c_uint64 * 3)()
    rc = load().rvcp_code_cache_counts(ctypes.cast(out, ctypes.c_void_p))
    if rc != RVCP_OK:
        raise RvcpError(rc, "rvcp_code_cache_counts failed")
    return dict(loads=int(out[0]), compiles=int(out[1]), rejects=int(out[2]))
