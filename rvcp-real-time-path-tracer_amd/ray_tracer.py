"""RayTracer: host-side mirror of the reference's ``Vk`` runtime (src/ray_tracer/vulkan.rs),
driving librvcp through its C-ABI.

    reference (vulkan.rs)                       here
    ------------------------------------------  -----------------------------------------
    Vk::new -> create_compute_pipeline (:576)   RayTracer(config)        -> rvcp_create
    create_descriptor_set_0s (:454-574)         RayTracer.upload_scene   -> rvcp_upload_scene
    create_command_buffers + dispatch (:406)    RayTracer.render         -> rvcp_render
    Vk::update_frame (:298-404)                 RayTracer.update_frame (render + FPS tick)

There is no CPU fallback: constructing a RayTracer without a HIP device or without the built
library raises.
"""
from __future__ import annotations

import ctypes
import time as _time
from typing import Optional

import numpy as np

from . import abi, scene_io
from .scene import CAMERA_DTYPE, PUSH_DTYPE, Scene, push_constant


class RayTracer:
    def __init__(self, config: Optional[np.ndarray] = None, **overrides):
        self._lib = abi.load()
        if config is None:
            config = abi.make_config(**overrides)
        self.config = np.ascontiguousarray(config)
        h = ctypes.c_void_p()
        rc = self._lib.rvcp_create(abi.ptr(self.config), ctypes.byref(h))
        if rc != abi.RVCP_OK:
            raise abi.RvcpError(rc, self._lib.rvcp_last_error(None).decode())
        self._ctx = h
        self.scene: Optional[Scene] = None
        self.last_stats = None
        self.last_temporal_ms = None
        self.last_denoise_ms = None
        self.last_svgf_accumulate_ms = None
        self.last_svgf_filter_ms = None
        self.last_rays_ms = None
        self.last_paths_ms = None
        self.last_paths_traversals = None
        # FPS counter (src/ray_tracer/ray_tracer.rs:80-86)
        self.fps_frame_count = 0
        self.fps_last_time = _time.perf_counter()
        self.fps = None

    # ------------------------------------------------------------------ lifetime
    def close(self):
        """rvcp_destroy; returns its code (RVCP_E_TIMEOUT: a gather was still stuck behind a
        collective at the deadline and the context's device memory was leaked, rvcp.h)."""
        rc = abi.RVCP_OK
        if getattr(self, "_ctx", None):
            rc = self._lib.rvcp_destroy(self._ctx)
            self._ctx = None
        return rc

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != abi.RVCP_OK:
            raise abi.RvcpError(rc, self._lib.rvcp_last_error(self._ctx).decode())

    @property
    def handle(self):
        return self._ctx

    # ------------------------------------------------------------------ scene
    def upload_arrays(self, materials, vertices, faces, lum_face_ids, spheres=None,
                      lum_sphere_ids=None):
        materials = np.ascontiguousarray(materials)
        vertices = np.ascontiguousarray(vertices)
        faces = np.ascontiguousarray(faces)
        lum = np.ascontiguousarray(lum_face_ids, dtype=np.uint32)
        sph = None if spheres is None or len(spheres) == 0 else np.ascontiguousarray(spheres)
        lsph = None if lum_sphere_ids is None or len(lum_sphere_ids) == 0 else \
            np.ascontiguousarray(lum_sphere_ids, dtype=np.uint32)
        self._check(self._lib.rvcp_upload_scene(
            self._ctx, abi.ptr(materials), len(materials), abi.ptr(vertices), len(vertices),
            abi.ptr(faces), len(faces), abi.ptr(sph), 0 if sph is None else len(sph),
            abi.ptr(lum), len(lum), abi.ptr(lsph), 0 if lsph is None else len(lsph)))

    def upload_scene(self, scene: Scene):
        self.upload_arrays(scene.aligned_materials(), scene.mesh.aligned_vertices(),
                           scene.mesh.aligned_faces(), scene.luminous_face_ids(),
                           scene.aligned_spheres(), scene.luminous_sphere_ids())
        self.scene = scene

    def upload_scene_file(self, path: str) -> np.ndarray:
        """Upload a binary scene file natively (rvcp_upload_scene_file); returns the stored
        AlignedCamera record and keeps the Python-side Scene for render()."""
        cam = np.zeros((), dtype=CAMERA_DTYPE)
        self._check(self._lib.rvcp_upload_scene_file(self._ctx, str(path).encode(), abi.ptr(cam)))
        self.scene = scene_io.load(path)
        return cam

    # ------------------------------------------------------------------ render
    def render_push(self, push: np.ndarray, width: int, height: int, want_linear: bool = False):
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        lin = np.empty((height, width, 3), dtype=np.float32) if want_linear else None
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        self._check(self._lib.rvcp_render(self._ctx, abi.ptr(push), width, height, abi.ptr(rgba),
                                          abi.ptr(lin), abi.ptr(stats)))
        self.last_stats = stats
        return (rgba, lin) if want_linear else rgba

    def render(self, width: int, height: int, time: float, want_linear: bool = False):
        if self.scene is None:
            raise RuntimeError("upload_scene first")
        return self.render_push(push_constant(self.scene.camera, time), width, height, want_linear)

    def update_frame(self, width: int, height: int, time: Optional[float] = None):
        """One frame of the interactive loop (vulkan.rs:298-404): time seed = unix secs % 1000
        (vulkan.rs:418-421) unless given; counts FPS like ray_tracer.rs:80-86."""
        if time is None:
            time = float(np.float32(_time.time() % 1000.0))
        img = self.render(width, height, time)
        self.fps_frame_count += 1
        now = _time.perf_counter()
        if now - self.fps_last_time >= 1.0:
            self.fps = self.fps_frame_count / (now - self.fps_last_time)
            self.fps_frame_count = 0
            self.fps_last_time = now
        return img

    def render_denoised(self, width: int, height: int, time: float, params=None,
                        want_linear: bool = False):
        """rvcp_render_denoised: one frame rendered, then filtered by the edge-avoiding a-trous
        denoiser under its own G-buffer (params: abi.make_denoise_params(...), None = the
        defaults).  Returns the filtered RGBA8 frame [, the filtered linear RGB]; last_stats are
        the render's and last_denoise_ms the filter's device time."""
        if self.scene is None:
            raise RuntimeError("upload_scene first")
        push = np.ascontiguousarray(push_constant(self.scene.camera, time), dtype=PUSH_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.DENOISE_PARAMS_DTYPE)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        lin = np.empty((height, width, 3), dtype=np.float32) if want_linear else None
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_render_denoised(
            self._ctx, abi.ptr(push), width, height, abi.ptr(params), abi.ptr(rgba), abi.ptr(lin),
            abi.ptr(stats), ctypes.cast(ctypes.byref(ms), ctypes.c_void_p)))
        self.last_stats = stats
        self.last_denoise_ms = float(ms.value)
        return (rgba, lin) if want_linear else rgba

    def render_temporal_push(self, push: np.ndarray, width: int, height: int, params=None,
                             denoise=None, want_linear: bool = False, want_history: bool = False):
        """rvcp_render_temporal for an explicit push constant (see render_temporal)."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TEMPORAL_PARAMS_DTYPE)
        if denoise is not None:
            denoise = np.ascontiguousarray(denoise, dtype=abi.DENOISE_PARAMS_DTYPE)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        lin = np.empty((height, width, 3), dtype=np.float32) if want_linear else None
        th, tw = self._traced_size(width, height)
        hist = np.empty((th, tw), dtype=np.uint32) if want_history else None
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        t_ms, d_ms = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.rvcp_render_temporal(
            self._ctx, abi.ptr(push), width, height, abi.ptr(params),
            abi.TEMPORAL_DENOISE if denoise is not None else 0, abi.ptr(denoise), abi.ptr(rgba),
            abi.ptr(lin), abi.ptr(hist), abi.ptr(stats),
            ctypes.cast(ctypes.byref(t_ms), ctypes.c_void_p),
            ctypes.cast(ctypes.byref(d_ms), ctypes.c_void_p)))
        self.last_stats = stats
        self.last_temporal_ms = float(t_ms.value)
        self.last_denoise_ms = float(d_ms.value)
        out = (rgba,) + ((lin,) if want_linear else ()) + ((hist,) if want_history else ())
        return out if len(out) > 1 else rgba

    def render_temporal(self, width: int, height: int, time: float, params=None, denoise=None,
                        want_linear: bool = False, want_history: bool = False):
        """rvcp_render_temporal: one frame rendered and blended into the history the context keeps
        from call to call, reprojected through the previous call's camera when the scene's camera
        moved (params: abi.make_temporal_params(...), None = the defaults).  denoise: an
        abi.make_denoise_params(...) record to show the a-trous filter of the accumulated frame
        (the history stays unfiltered); None: no spatial pass.  Returns the RGBA8 frame [, its
        linear RGB] [, the per-pixel history lengths]; last_stats are the render's,
        last_temporal_ms / last_denoise_ms the device times of the two steps.  The history restarts
        on a size change, upload_scene and temporal_reset()."""
        if self.scene is None:
            raise RuntimeError("upload_scene first")
        return self.render_temporal_push(push_constant(self.scene.camera, time), width, height,
                                         params, denoise, want_linear, want_history)

    def temporal_reset(self):
        """rvcp_temporal_reset: drop the history render_temporal keeps."""
        self._check(self._lib.rvcp_temporal_reset(self._ctx))

    def render_svgf_push(self, push: np.ndarray, width: int, height: int, params=None, svgf=None,
                         feedback: bool = False, want_linear: bool = False,
                         want_variance: bool = False, want_history: bool = False):
        """rvcp_render_svgf for an explicit push constant (see render_svgf)."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TEMPORAL_PARAMS_DTYPE)
        if svgf is not None:
            svgf = np.ascontiguousarray(svgf, dtype=abi.SVGF_PARAMS_DTYPE)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        lin = np.empty((height, width, 3), dtype=np.float32) if want_linear else None
        th, tw = self._traced_size(width, height)
        var = np.empty((th, tw), dtype=np.float32) if want_variance else None
        hist = np.empty((th, tw), dtype=np.uint32) if want_history else None
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        a_ms, f_ms = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.rvcp_render_svgf(
            self._ctx, abi.ptr(push), width, height, abi.ptr(params), abi.ptr(svgf),
            abi.SVGF_FEEDBACK if feedback else 0, abi.ptr(rgba), abi.ptr(lin), abi.ptr(var),
            abi.ptr(hist), abi.ptr(stats), ctypes.cast(ctypes.byref(a_ms), ctypes.c_void_p),
            ctypes.cast(ctypes.byref(f_ms), ctypes.c_void_p)))
        self.last_stats = stats
        self.last_svgf_accumulate_ms = float(a_ms.value)
        self.last_svgf_filter_ms = float(f_ms.value)
        out = (rgba,) + ((lin,) if want_linear else ()) + ((var,) if want_variance else ()) + \
            ((hist,) if want_history else ())
        return out if len(out) > 1 else rgba

    def render_svgf(self, width: int, height: int, time: float, params=None, svgf=None,
                    feedback: bool = False, want_linear: bool = False,
                    want_variance: bool = False, want_history: bool = False):
        """rvcp_render_svgf: one frame rendered, blended with its luminance moments into the SVGF
        history the context keeps (apart from render_temporal's), turned into a per-pixel variance
        and filtered by the variance-guided a-trous passes (params: abi.make_temporal_params(...),
        svgf: abi.make_svgf_params(...); None = the defaults).  feedback: the next frame's colour
        history is pass 0's output.  Returns the RGBA8 frame [, its linear RGB] [, its variance]
        [, the history lengths]; last_stats are the render's, last_svgf_accumulate_ms /
        last_svgf_filter_ms the device times of the two steps.  The history restarts on a size
        change, upload_scene and svgf_reset()."""
        if self.scene is None:
            raise RuntimeError("upload_scene first")
        return self.render_svgf_push(push_constant(self.scene.camera, time), width, height, params,
                                     svgf, feedback, want_linear, want_variance, want_history)

    def svgf_reset(self):
        """rvcp_svgf_reset: drop the history render_svgf keeps."""
        self._check(self._lib.rvcp_svgf_reset(self._ctx))

    def mandelbrot(self, push: np.ndarray, width: int, height: int, want_value: bool = False):
        """The Mandelbrot operator (rvcp_mandelbrot): grey RGBA8 frame [, escape values]."""
        from .mandelbrot import MANDELBROT_PUSH_DTYPE
        push = np.ascontiguousarray(push, dtype=MANDELBROT_PUSH_DTYPE)
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        val = np.empty((height, width), dtype=np.float32) if want_value else None
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        self._check(self._lib.rvcp_mandelbrot(self._ctx, abi.ptr(push), width, height,
                                              abi.ptr(rgba), abi.ptr(val), abi.ptr(stats)))
        self.last_stats = stats
        return (rgba, val) if want_value else rgba

    # ------------------------------------------------------------------ device-side API
    def render_shard_async(self, push, width, height, shard_index, shard_count, d_rgba: int,
                           d_linear: int = 0, stream: int = 0):
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._push_keepalive = push
        self._check(self._lib.rvcp_render_shard_async(
            self._ctx, abi.ptr(push), width, height, shard_index, shard_count,
            ctypes.c_void_p(d_rgba), ctypes.c_void_p(d_linear) if d_linear else None,
            ctypes.c_void_p(stream) if stream else None))

    def render_frames_async(self, pushes, width, height, shard_index, shard_count, d_rgba: int,
                            d_linear: int = 0, stream: int = 0):
        """rvcp_render_frames_async: a batch of len(pushes) consecutive frames of one shard in
        one path kernel; frame k's rows start at pixel k * shard_rows(height, 0, shard_count) *
        width of d_rgba (and of d_linear).  Wait with sync_stats() / wait()."""
        pushes = np.ascontiguousarray(pushes, dtype=PUSH_DTYPE).reshape(-1)
        self._push_keepalive = pushes
        self._check(self._lib.rvcp_render_frames_async(
            self._ctx, abi.ptr(pushes), len(pushes), width, height, shard_index, shard_count,
            ctypes.c_void_p(d_rgba), ctypes.c_void_p(d_linear) if d_linear else None,
            ctypes.c_void_p(stream) if stream else None))

    def render_async(self, push, width, height, d_rgba: int, d_linear: int = 0, stream: int = 0):
        """rvcp_render_async: enqueue one full frame into device memory; see wait()."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._push_keepalive = push
        self._check(self._lib.rvcp_render_async(
            self._ctx, abi.ptr(push), width, height, ctypes.c_void_p(d_rgba),
            ctypes.c_void_p(d_linear) if d_linear else None,
            ctypes.c_void_p(stream) if stream else None))

    def render_gbuffer_async(self, push, width, height, d_gbuffer: int, stream: int = 0):
        """rvcp_render_gbuffer_async: enqueue the frame's G-buffer (width * height records of
        abi.GBUFFER_DTYPE) into device memory; ordered on the stream, nothing to wait for."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._check(self._lib.rvcp_render_gbuffer_async(
            self._ctx, abi.ptr(push), width, height, ctypes.c_void_p(d_gbuffer),
            ctypes.c_void_p(stream) if stream else None))

    def denoise_async(self, d_linear_in: int, d_gbuffer: int, width, height, d_linear_out: int,
                      d_rgba: int = 0, params=None, stream: int = 0):
        """rvcp_denoise_async: enqueue the a-trous filter of a linear-RGB frame in device memory
        under a G-buffer; the filtered floats go to d_linear_out (no overlap with the input) and,
        when given, their gamma / UNORM8 bytes to d_rgba.  Wait with denoise_wait()."""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.DENOISE_PARAMS_DTYPE)
        self._check(self._lib.rvcp_denoise_async(
            self._ctx, ctypes.c_void_p(d_linear_in), ctypes.c_void_p(d_gbuffer), width, height,
            abi.ptr(params), ctypes.c_void_p(d_linear_out),
            ctypes.c_void_p(d_rgba) if d_rgba else None,
            ctypes.c_void_p(stream) if stream else None))

    def denoise_wait(self) -> float:
        """rvcp_denoise_wait: block until the last denoise_async is done; its device time, ms."""
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_denoise_wait(self._ctx, ctypes.cast(ctypes.byref(ms),
                                                                       ctypes.c_void_p)))
        return float(ms.value)

    # ------------------------------------------------------------------ ray queries (§4.19)
    def trace_rays_async(self, d_rays: int, n: int, d_out: int, mode: int = abi.RAYS_NEAREST,
                         stream: int = 0):
        """rvcp_trace_rays_async: enqueue a query of n abi.RAY_DTYPE rays in device memory;
        d_out gets n abi.RAY_HIT_DTYPE records (RAYS_NEAREST) or n uint32 (RAYS_ANY).  Wait with
        rays_wait()."""
        P = ctypes.c_void_p
        self._check(self._lib.rvcp_trace_rays_async(
            self._ctx, P(d_rays) if d_rays else None, n, mode, P(d_out) if d_out else None,
            P(stream) if stream else None))

    def rays_wait(self) -> float:
        """rvcp_rays_wait: block until the last trace_rays_async is done; its device time, ms."""
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_rays_wait(self._ctx, ctypes.cast(ctypes.byref(ms),
                                                                    ctypes.c_void_p)))
        return float(ms.value)

    def trace_rays(self, rays, mode: int = abi.RAYS_NEAREST) -> np.ndarray:
        """rvcp_trace_rays: rays (abi.RAY_DTYPE records) from host memory, synchronously; returns
        abi.RAY_HIT_DTYPE records (RAYS_NEAREST) or uint32 (RAYS_ANY) and sets last_rays_ms."""
        rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE).reshape(-1)
        out = np.empty(len(rays), dtype=np.uint32 if mode == abi.RAYS_ANY else abi.RAY_HIT_DTYPE)
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_trace_rays(
            self._ctx, abi.ptr(rays), len(rays), mode, abi.ptr(out),
            ctypes.cast(ctypes.byref(ms), ctypes.c_void_p)))
        self.last_rays_ms = float(ms.value)
        return out

    def primary_rays_async(self, push, width, height, d_rays: int, stream: int = 0):
        """rvcp_primary_rays_async: enqueue the frame's width * height primary rays
        (abi.RAY_DTYPE, pixel order) into device memory; ordered on the stream."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._check(self._lib.rvcp_primary_rays_async(
            self._ctx, abi.ptr(push), width, height, ctypes.c_void_p(d_rays) if d_rays else None,
            ctypes.c_void_p(stream) if stream else None))

    def pick(self, width: int, height: int, x: int, y: int, time: float = 0.0) -> np.ndarray:
        """rvcp_pick: the nearest hit (one abi.RAY_HIT_DTYPE record) under pixel (x, y) of the
        width x height frame through the uploaded scene's camera."""
        if self.scene is None:
            raise RuntimeError("upload_scene first")
        push = np.ascontiguousarray(push_constant(self.scene.camera, time), dtype=PUSH_DTYPE)
        hit = np.zeros((), dtype=abi.RAY_HIT_DTYPE)
        self._check(self._lib.rvcp_pick(self._ctx, abi.ptr(push), width, height, x, y,
                                        abi.ptr(hit)))
        return hit

    # ------------------------------------------------------------------ path queries (§4.20)
    def trace_paths_async(self, d_rays: int, d_seeds: int, n: int, spp: int, d_out: int,
                          stream: int = 0):
        """rvcp_trace_paths_async: enqueue a query of n abi.RAY_DTYPE rays and n float32 seeds in
        device memory, spp samples per ray; d_out gets n x 3 float32 of linear RGB.  Wait with
        paths_wait()."""
        P = ctypes.c_void_p
        self._check(self._lib.rvcp_trace_paths_async(
            self._ctx, P(d_rays) if d_rays else None, P(d_seeds) if d_seeds else None, n, spp,
            P(d_out) if d_out else None, P(stream) if stream else None))

    def paths_wait(self):
        """rvcp_paths_wait: block until the last trace_paths_async is done; (its device time in
        ms, the traversals it made)."""
        ms = ctypes.c_float(0.0)
        trav = ctypes.c_uint64(0)
        self._check(self._lib.rvcp_paths_wait(self._ctx,
                                              ctypes.cast(ctypes.byref(ms), ctypes.c_void_p),
                                              ctypes.cast(ctypes.byref(trav), ctypes.c_void_p)))
        return float(ms.value), int(trav.value)

    def trace_paths(self, rays, seeds=None, spp: Optional[int] = None, seed: int = 0) -> np.ndarray:
        """rvcp_trace_paths: the radiance along rays (abi.RAY_DTYPE records) from host memory,
        synchronously: an (n, 3) float32 array of linear RGB.  seeds: one float32 in [0, 1) per
        ray, or None to draw them from numpy.random.default_rng(seed); spp: samples per ray, or
        None for the context's.  Sets last_paths_ms and last_paths_traversals."""
        rays = np.ascontiguousarray(rays, dtype=abi.RAY_DTYPE).reshape(-1)
        if seeds is None:
            seeds = np.random.default_rng(seed).random(len(rays), dtype=np.float32)
        seeds = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1)
        if len(seeds) != len(rays):
            raise ValueError("one seed per ray")
        if spp is None:
            spp = int(np.asarray(self.config["spp"]).reshape(-1)[0])
        out = np.empty((len(rays), 3), dtype=np.float32)
        ms = ctypes.c_float(0.0)
        trav = ctypes.c_uint64(0)
        self._check(self._lib.rvcp_trace_paths(
            self._ctx, abi.ptr(rays), abi.ptr(seeds), len(rays), spp, abi.ptr(out),
            ctypes.cast(ctypes.byref(ms), ctypes.c_void_p),
            ctypes.cast(ctypes.byref(trav), ctypes.c_void_p)))
        self.last_paths_ms = float(ms.value)
        self.last_paths_traversals = int(trav.value)
        return out

    def primary_seeds_async(self, push, width, height, d_seeds: int, stream: int = 0):
        """rvcp_primary_seeds_async: enqueue the frame's width * height pixel seeds (float32,
        pixel order) into device memory; ordered on the stream."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._check(self._lib.rvcp_primary_seeds_async(
            self._ctx, abi.ptr(push), width, height, ctypes.c_void_p(d_seeds) if d_seeds else None,
            ctypes.c_void_p(stream) if stream else None))

    def temporal_accumulate_async(self, view, d_cur_linear: int, d_cur_gbuffer: int,
                                  d_prev_linear: int, d_prev_gbuffer: int, d_prev_len: int,
                                  width, height, d_out_linear: int, d_out_len: int,
                                  d_rgba: int = 0, params=None, stream: int = 0):
        """rvcp_temporal_accumulate_async: enqueue one accumulation step on frames in device
        memory.  view: the previous frame's abi.temporal_view(...) record, or None when the camera
        did not move; d_prev_* all 0: no history.  Wait with temporal_wait()."""
        if view is not None:
            view = np.ascontiguousarray(view, dtype=abi.TEMPORAL_VIEW_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TEMPORAL_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_temporal_accumulate_async(
            self._ctx, abi.ptr(view), P(d_cur_linear), P(d_cur_gbuffer), P(d_prev_linear),
            P(d_prev_gbuffer), P(d_prev_len), width, height, abi.ptr(params), P(d_out_linear),
            P(d_out_len), P(d_rgba), P(stream)))

    def temporal_wait(self) -> float:
        """rvcp_temporal_wait: block until the last temporal_accumulate_async is done; its device
        time, ms."""
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_temporal_wait(self._ctx, ctypes.cast(ctypes.byref(ms),
                                                                        ctypes.c_void_p)))
        return float(ms.value)

    def svgf_accumulate_async(self, view, d_cur_linear: int, d_cur_gbuffer: int,
                              d_prev_linear: int, d_prev_gbuffer: int, d_prev_len: int,
                              d_prev_moments: int, width, height, d_out_linear: int,
                              d_out_len: int, d_out_moments: int, d_rgba: int = 0, params=None,
                              svgf=None, stream: int = 0):
        """rvcp_svgf_accumulate_async: temporal_accumulate_async that also carries the luminance
        moments (width * height float pairs); d_prev_* all 0: no history.  Wait with
        svgf_wait()."""
        if view is not None:
            view = np.ascontiguousarray(view, dtype=abi.TEMPORAL_VIEW_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TEMPORAL_PARAMS_DTYPE)
        if svgf is not None:
            svgf = np.ascontiguousarray(svgf, dtype=abi.SVGF_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_svgf_accumulate_async(
            self._ctx, abi.ptr(view), P(d_cur_linear), P(d_cur_gbuffer), P(d_prev_linear),
            P(d_prev_gbuffer), P(d_prev_len), P(d_prev_moments), width, height, abi.ptr(params),
            abi.ptr(svgf), P(d_out_linear), P(d_out_len), P(d_out_moments), P(d_rgba), P(stream)))

    def svgf_filter_async(self, d_linear: int, d_moments: int, d_len: int, d_gbuffer: int, width,
                          height, d_linear_out: int, d_variance_out: int = 0,
                          d_feedback_out: int = 0, d_rgba: int = 0, svgf=None, stream: int = 0):
        """rvcp_svgf_filter_async: variance estimate, guided a-trous passes and tone map of an
        accumulated frame in device memory; optional outputs are 0.  Wait with svgf_wait()."""
        if svgf is not None:
            svgf = np.ascontiguousarray(svgf, dtype=abi.SVGF_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_svgf_filter_async(
            self._ctx, P(d_linear), P(d_moments), P(d_len), P(d_gbuffer), width, height,
            abi.ptr(svgf), P(d_linear_out), P(d_variance_out), P(d_feedback_out), P(d_rgba),
            P(stream)))

    def svgf_wait(self):
        """rvcp_svgf_wait: block until the last svgf_accumulate_async / svgf_filter_async are done;
        their device times (accumulate_ms, filter_ms), 0 for a step that was not enqueued."""
        a, f = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.rvcp_svgf_wait(self._ctx, ctypes.cast(ctypes.byref(a), ctypes.c_void_p),
                                             ctypes.cast(ctypes.byref(f), ctypes.c_void_p)))
        return float(a.value), float(f.value)

    # albedo demodulation
    @property
    def demodulation(self) -> bool:
        """The context's demodulation switch (rvcp_get_demodulation / rvcp_set_demodulation):
        while True, render_denoised, render_temporal and render_svgf filter irradiance (colour /
        albedo of the primary hit) and multiply the albedo back in their store.  Changing it
        drops both histories."""
        on = ctypes.c_int(0)
        self._check(self._lib.rvcp_get_demodulation(self._ctx, ctypes.cast(ctypes.byref(on),
                                                                          ctypes.c_void_p)))
        return bool(on.value)

    @demodulation.setter
    def demodulation(self, on: bool):
        self._check(self._lib.rvcp_set_demodulation(self._ctx, 1 if on else 0))

    def demodulate_async(self, d_linear: int, d_gbuffer: int, width, height,
                         d_irradiance_out: int, stream: int = 0):
        """rvcp_demodulate_async: enqueue colour / albedo of a linear-RGB frame in device memory
        under a G-buffer; d_irradiance_out may be d_linear itself.  Wait with albedo_wait()."""
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_demodulate_async(
            self._ctx, P(d_linear), P(d_gbuffer), width, height, P(d_irradiance_out), P(stream)))

    def remodulate_async(self, d_irradiance: int, d_gbuffer: int, width, height,
                         d_linear_out: int = 0, d_rgba: int = 0, stream: int = 0):
        """rvcp_remodulate_async: enqueue irradiance x albedo fused with the store: the linear
        colour to d_linear_out and / or its gamma / UNORM8 bytes to d_rgba (one of them may be
        0).  Wait with albedo_wait()."""
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_remodulate_async(
            self._ctx, P(d_irradiance), P(d_gbuffer), width, height, P(d_linear_out), P(d_rgba),
            P(stream)))

    def albedo_wait(self):
        """rvcp_albedo_wait: block until the last demodulate_async / remodulate_async are done;
        their device times (demodulate_ms, remodulate_ms), 0 for a step that was not enqueued."""
        d, r = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.rvcp_albedo_wait(self._ctx, ctypes.cast(ctypes.byref(d), ctypes.c_void_p),
                                               ctypes.cast(ctypes.byref(r), ctypes.c_void_p)))
        return float(d.value), float(r.value)

    # temporal anti-aliasing
    @property
    def taa(self) -> bool:
        """The context's TAA switch (rvcp_get_taa / rvcp_set_taa): while True, render_temporal and
        render_svgf render through a camera jittered by abi.taa_jitter(frame counter) and return
        the resolved frame (taa_resolve_async of their final linear colour under the unjittered
        cameras).  Changing it drops both chains' histories."""
        on = ctypes.c_int(0)
        self._check(self._lib.rvcp_get_taa(self._ctx, ctypes.cast(ctypes.byref(on), ctypes.c_void_p)))
        return bool(on.value)

    @taa.setter
    def taa(self, on: bool):
        self._check(self._lib.rvcp_set_taa(self._ctx, 1 if on else 0))

    def taa_reset(self):
        """rvcp_taa_reset: drop the TAA states render_temporal and render_svgf keep; their jitter
        sequences restart."""
        self._check(self._lib.rvcp_taa_reset(self._ctx))

    def taa_resolve_async(self, cur_view, prev_view, d_cur_linear: int, d_cur_gbuffer: int,
                          d_prev_resolved: int, d_prev_len: int, width, height,
                          d_out_resolved: int, d_out_len: int, d_rgba: int = 0, params=None,
                          stream: int = 0):
        """rvcp_taa_resolve_async: enqueue one resolve step on frames in device memory.  cur_view /
        prev_view: the abi.temporal_view(...) records of the two frames' UNJITTERED cameras, or
        both None when the camera is at rest; d_prev_* both 0: no history.  Wait with
        taa_wait()."""
        if cur_view is not None:
            cur_view = np.ascontiguousarray(cur_view, dtype=abi.TEMPORAL_VIEW_DTYPE)
        if prev_view is not None:
            prev_view = np.ascontiguousarray(prev_view, dtype=abi.TEMPORAL_VIEW_DTYPE)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TAA_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_taa_resolve_async(
            self._ctx, abi.ptr(cur_view), abi.ptr(prev_view), P(d_cur_linear), P(d_cur_gbuffer),
            P(d_prev_resolved), P(d_prev_len), width, height, abi.ptr(params), P(d_out_resolved),
            P(d_out_len), P(d_rgba), P(stream)))

    def taa_wait(self) -> float:
        """rvcp_taa_wait: block until the last taa_resolve_async is done; its device time, ms."""
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_taa_wait(self._ctx, ctypes.cast(ctypes.byref(ms), ctypes.c_void_p)))
        return float(ms.value)

    # temporal upsampling
    @property
    def taa_upsample(self) -> int:
        """The context's upsampling scale (rvcp_get_taa_upsample / rvcp_set_taa_upsample): 1 (off),
        2, 3 or 4.  While it is above 1, render_temporal and render_svgf trace width / scale x
        height / scale pixels through the jittered camera and return the width x height frame
        that taa_upsample_async accumulates (it replaces the TAA resolve); the history lengths and
        the variance keep the traced size.  Changing it drops both chains' histories."""
        scale = ctypes.c_uint32(0)
        self._check(self._lib.rvcp_get_taa_upsample(self._ctx, ctypes.cast(ctypes.byref(scale),
                                                                          ctypes.c_void_p)))
        return int(scale.value)

    @taa_upsample.setter
    def taa_upsample(self, scale: int):
        self._check(self._lib.rvcp_set_taa_upsample(self._ctx, int(scale)))

    # bounce sampling of the games101 integrator
    @property
    def sampling(self) -> int:
        """The context's bounce sampling (rvcp_get_sampling / rvcp_set_sampling):
        abi.SAMPLING_UNIFORM (the default: the shader's bounce, frames bit-identical to the
        oracle) or abi.SAMPLING_COSINE (cosine-weighted directions with the constant weight
        albedo / rr: less noise per sample, frames no longer the oracle's).  It holds from the
        next render on, across upload_scene; changing it drops the temporal chains' histories."""
        mode = ctypes.c_int32(0)
        self._check(self._lib.rvcp_get_sampling(self._ctx, ctypes.cast(ctypes.byref(mode),
                                                                      ctypes.c_void_p)))
        return int(mode.value)

    @sampling.setter
    def sampling(self, mode: int):
        self._check(self._lib.rvcp_set_sampling(self._ctx, int(mode)))

    # material scattering on meshes
    @property
    def materials(self) -> int:
        """The context's materials mode (rvcp_get_materials / rvcp_set_materials):
        abi.MATERIALS_LAMBERTIAN (the default: every non-emissive face is a Lambertian surface,
        as in the shader; frames bit-identical to the oracle) or abi.MATERIALS_SCATTER (Metal
        and Dielectric faces reflect and refract as the reference's material_scatter defines;
        render, the chains and trace_paths run the material kernel).  It holds across
        upload_scene, which then rejects a fuzz outside [0, 1] or a refraction ratio that is
        not positive; changing it drops the temporal chains' histories."""
        mode = ctypes.c_int32(0)
        self._check(self._lib.rvcp_get_materials(self._ctx, ctypes.cast(ctypes.byref(mode),
                                                                       ctypes.c_void_p)))
        return int(mode.value)

    @materials.setter
    def materials(self, mode: int):
        self._check(self._lib.rvcp_set_materials(self._ctx, int(mode)))

    # adaptive sampling: per-pixel sample counts
    def render_spp_map_async(self, push, width, height, d_spp_map: int, spp_hint: int, d_rgba: int,
                             d_linear: int = 0, stream: int = 0):
        """rvcp_render_spp_map_async: render_async with a per-pixel sample count -- d_spp_map holds
        width * height uint32 in device memory, each clamped to 1..abi.SPP_MAP_MAX by the kernel;
        cfg.spp is not read and spp_hint (1..abi.SPP_MAP_MAX) only steers the schedule and the
        grid.  Every pixel is bit for bit the pixel of a frame rendered at spp = its count.  Wait
        with wait() / sync_stats()."""
        push = np.ascontiguousarray(push, dtype=PUSH_DTYPE)
        self._push_keepalive = push
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_render_spp_map_async(
            self._ctx, abi.ptr(push), width, height, P(d_spp_map), int(spp_hint), P(d_rgba),
            P(d_linear), P(stream)))

    def spp_plan_async(self, d_variance: int, d_linear: int, d_len: int, d_gbuffer: int, width,
                       height, d_spp_map_out: int, params=None, stream: int = 0):
        """rvcp_spp_plan_async: enqueue the plan step -- the next frame's map (width * height
        uint32 into d_spp_map_out) from a frame's variance, the colour it belongs to, its history
        lengths (d_len 0: 1 everywhere) and its G-buffer, all in device memory (params:
        abi.make_adaptive_params(...); None = the defaults).  Wait with spp_plan_wait()."""
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.ADAPTIVE_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_spp_plan_async(
            self._ctx, P(d_variance), P(d_linear), P(d_len), P(d_gbuffer), width, height,
            abi.ptr(params), P(d_spp_map_out), P(stream)))

    def spp_plan_wait(self):
        """rvcp_spp_plan_wait: block until the last spp_plan_async is done; (its device time in
        ms, the sum of the map it wrote)."""
        ms, total = ctypes.c_float(0.0), ctypes.c_uint64(0)
        self._check(self._lib.rvcp_spp_plan_wait(
            self._ctx, ctypes.cast(ctypes.byref(ms), ctypes.c_void_p),
            ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
        return float(ms.value), int(total.value)

    @property
    def adaptive(self):
        """The adaptive-sampling switch (rvcp_get_adaptive / rvcp_set_adaptive): None (off, the
        default) or its abi.ADAPTIVE_PARAMS_DTYPE parameters.  While it is on, render_svgf traces
        each frame through the per-pixel counts planned from the previous frame's variance (a
        uniform map wherever its history restarts).  Setting it (params, or None for off) drops
        the map, not the SVGF history."""
        on = ctypes.c_int(0)
        p = np.zeros((), dtype=abi.ADAPTIVE_PARAMS_DTYPE)
        self._check(self._lib.rvcp_get_adaptive(
            self._ctx, ctypes.cast(ctypes.byref(on), ctypes.c_void_p), abi.ptr(p)))
        return p if on.value else None

    @adaptive.setter
    def adaptive(self, params):
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.ADAPTIVE_PARAMS_DTYPE)
            self._adaptive_keepalive = params
        self._check(self._lib.rvcp_set_adaptive(self._ctx, abi.ptr(params)))

    def adaptive_last_map(self) -> np.ndarray:
        """rvcp_adaptive_last_map: the (rows, columns) uint32 map the last render_svgf frame was
        traced with under the adaptive switch."""
        w, h = ctypes.c_uint32(0), ctypes.c_uint32(0)
        pw = ctypes.cast(ctypes.byref(w), ctypes.c_void_p)
        ph = ctypes.cast(ctypes.byref(h), ctypes.c_void_p)
        self._check(self._lib.rvcp_adaptive_last_map(self._ctx, None, pw, ph))
        out = np.empty((h.value, w.value), dtype=np.uint32)
        self._check(self._lib.rvcp_adaptive_last_map(self._ctx, abi.ptr(out), pw, ph))
        return out

    def _traced_size(self, width, height):
        """(rows, columns) of the frame render_temporal / render_svgf trace for a width x height
        call: the optional outputs other than the frame itself have this size."""
        s = self.taa_upsample
        if s > 1 and width % s == 0 and height % s == 0:
            return height // s, width // s
        return height, width

    def taa_upsample_async(self, scale: int, jit_view, cur_view, prev_view, d_cur_linear: int,
                           d_gbuffer_hi: int, d_prev_resolved: int, d_prev_weight: int, width,
                           height, d_out_resolved: int, d_out_weight: int, d_rgba: int = 0,
                           params=None, stream: int = 0):
        """rvcp_taa_upsample_async: enqueue one upsampling step of a width x height frame from a
        frame traced at width / scale x height / scale in device memory.  jit_view: the
        abi.temporal_view(...) record of the jittered camera at the traced size; cur_view /
        prev_view: those of the UNJITTERED cameras at width x height (prev_view None: the camera is
        at rest); d_gbuffer_hi: the width x height G-buffer through the unjittered camera, needed
        when the camera moved, else 0; d_prev_* both 0: no history.  Wait with taau_wait()."""
        views = [None if v is None else np.ascontiguousarray(v, dtype=abi.TEMPORAL_VIEW_DTYPE)
                 for v in (jit_view, cur_view, prev_view)]
        if params is not None:
            params = np.ascontiguousarray(params, dtype=abi.TAAU_PARAMS_DTYPE)
        P = lambda a: ctypes.c_void_p(a) if a else None   # noqa: E731
        self._check(self._lib.rvcp_taa_upsample_async(
            self._ctx, scale, abi.ptr(views[0]), abi.ptr(views[1]), abi.ptr(views[2]),
            P(d_cur_linear), P(d_gbuffer_hi), P(d_prev_resolved), P(d_prev_weight), width, height,
            abi.ptr(params), P(d_out_resolved), P(d_out_weight), P(d_rgba), P(stream)))

    def taau_wait(self) -> float:
        """rvcp_taau_wait: block until the last taa_upsample_async is done; its device time, ms."""
        ms = ctypes.c_float(0.0)
        self._check(self._lib.rvcp_taau_wait(self._ctx, ctypes.cast(ctypes.byref(ms), ctypes.c_void_p)))
        return float(ms.value)

    def wait(self):
        """rvcp_wait: block until the last async render is done; returns its stats."""
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        self._check(self._lib.rvcp_wait(self._ctx, abi.ptr(stats)))
        self.last_stats = stats
        return stats

    def sync_stats(self):
        stats = np.zeros((), dtype=abi.STATS_DTYPE)
        self._check(self._lib.rvcp_sync_stats(self._ctx, abi.ptr(stats)))
        self.last_stats = stats
        return stats

    def assemble_frame_async(self, d_gathered: int, slot_rows: int, width: int, height: int,
                             shard_count: int, d_frame: int, stream: int = 0):
        self._check(self._lib.rvcp_assemble_frame_async(
            self._ctx, ctypes.c_void_p(d_gathered), slot_rows, width, height, shard_count,
            ctypes.c_void_p(d_frame), ctypes.c_void_p(stream) if stream else None))

    # ------------------------------------------------------------------ one process per GPU
    def rccl_init(self, unique_id: bytes, world: int, rank: int):
        """rvcp_rccl_init: join the frame-gather communicator (collective over `world` ranks;
        `unique_id` from rccl_unique_id() on rank 0, shared out of band)."""
        if len(unique_id) != abi.RCCL_ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        buf = (ctypes.c_uint8 * abi.RCCL_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.rvcp_rccl_init(self._ctx, ctypes.cast(buf, ctypes.c_void_p), world, rank))

    def rccl_attach(self, nccl_comm: int, world: int, rank: int):
        """rvcp_rccl_attach: gather over the caller's communicator (an ncclComm_t on this
        context's device; blocking or not); the caller keeps it and is the one to abort it."""
        self._check(self._lib.rvcp_rccl_attach(self._ctx, ctypes.c_void_p(nccl_comm), world, rank))

    def rccl_set_timeout(self, timeout_ms: int):
        """rvcp_rccl_set_timeout: deadline of rccl_init / gather_wait in ms (0 = none); past it
        they raise RvcpError with code RVCP_E_TIMEOUT and the communicator is aborted."""
        self._check(self._lib.rvcp_rccl_set_timeout(self._ctx, int(timeout_ms)))

    def gather_frame_async(self, d_shard: int, width: int, height: int, d_gathered: int = 0,
                           d_frame: int = 0, stream: int = 0):
        """rvcp_gather_frame_async: RCCL gather of the shards to rank 0 + device assembly
        there (d_gathered / d_frame only on rank 0)."""
        self._check(self._lib.rvcp_gather_frame_async(
            self._ctx, ctypes.c_void_p(d_shard), width, height,
            ctypes.c_void_p(d_gathered) if d_gathered else None,
            ctypes.c_void_p(d_frame) if d_frame else None,
            ctypes.c_void_p(stream) if stream else None))

    def gather_wait(self):
        """rvcp_gather_wait: block until the last gather is done; returns (gather_ms,
        render-start-to-gather-end ms) from HIP events on the gather's stream."""
        g, f = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._lib.rvcp_gather_wait(self._ctx, ctypes.byref(g), ctypes.byref(f)))
        return float(g.value), float(f.value)


def rccl_unique_id() -> bytes:
    """rvcp_rccl_unique_id (rank 0): the 128-byte RCCL communicator id."""
    L = abi.load()
    buf = (ctypes.c_uint8 * abi.RCCL_ID_BYTES)()
    rc = L.rvcp_rccl_unique_id(ctypes.cast(buf, ctypes.c_void_p))
    if rc != abi.RVCP_OK:
        raise abi.RvcpError(rc, L.rvcp_last_error(None).decode())
    return bytes(buf)


def shard_rows(height: int, shard_index: int, shard_count: int) -> int:
    """Rows of shard `shard_index` (8-row stripes dealt round-robin).  Pure-Python twin of
    rvcp_shard_rows for hosts without the library loaded."""
    stripes = (height + 7) // 8
    return sum(min(8, height - 8 * s) for s in range(shard_index, stripes, shard_count))


def shard_row_ids(height: int, shard_index: int, shard_count: int) -> np.ndarray:
    """Global row ids of a shard's packed rows, in order."""
    stripes = (height + 7) // 8
    rows = [y for s in range(shard_index, stripes, shard_count)
            for y in range(8 * s, min(8 * s + 8, height))]
    return np.array(rows, dtype=np.int64)
