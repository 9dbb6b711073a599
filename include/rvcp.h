/*
 * rvcp.h -- C-ABI of librvcp, the MI355X (gfx950) replacement for the Vulkano compute
 * pipeline of YXHXianYu/RVCP-Real-Time-Path-Tracer (`src/ray_tracer/vulkan.rs`).
 *
 * The hot path behind this ABI is the per-pixel path-tracing kernel that `src/ray_tracer`
 * dispatches: `assets/shaders/ray_tracer_games101_branch.comp` (selected by
 * `src/ray_tracer/shader.rs:12`).  Every struct below is byte-identical to the reference's
 * Rust-side upload struct (`#[repr(C)]`, `BufferContents`), so a Rust caller can hand the
 * same `Vec<Aligned*>` it used to give `Buffer::from_iter` straight to this library.
 *
 * Conventions
 *   - All functions return 0 (RVCP_OK) on success and a negative RVCP_E_* code on failure.
 *     Nothing aborts or throws across the ABI; `rvcp_last_error(ctx)` returns a message.
 *   - A context is not thread-safe: use one context per host thread.
 *   - One frame in flight per context: a render, upload or Mandelbrot call while an async
 *     frame is pending (rvcp_render_async / rvcp_render_shard_async not yet waited for with
 *     rvcp_wait / rvcp_sync_stats) fails with RVCP_E_INVALID.  Use one context per frame in
 *     flight.
 *   - Host pointers stay owned by the caller; the library copies what it needs.
 *   - Pointers named `d_*` are HIP device pointers; `stream` is a `hipStream_t` (NULL = the
 *     context's own stream, created by rvcp_create).
 */
#ifndef RVCP_H
#define RVCP_H

#ifndef __HIPCC_RTC__               /* hipRTC (the scene-specialised kernels) has these built in */
#include <stddef.h>
#include <stdint.h>
#else
using __hip_internal::int32_t;
using __hip_internal::uint8_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#ifndef offsetof
#define offsetof(t, m) __builtin_offsetof(t, m)
#endif
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Upload structs (byte-identical to the reference; RVCP_STATIC_ASSERTs below)
 * ------------------------------------------------------------------------------------- */

/* == AlignedCamera, src/ray_tracer/scene/camera.rs:27-37 (64 B).
 *    Shader view: struct Camera, ray_tracer_games101_branch.comp:37-44 (std430 push block). */
typedef struct rvcp_camera {
    float position[4];      /* xyz + pad (utils.rs:5-7 vec3_to_f32_4) */
    float up[4];            /* xyz + pad */
    float forward[3];
    float t_near;
    float t_far;
    float vertical_fov;     /* degrees */
    uint32_t _padding[2];
} rvcp_camera_t;

/* == PushConstant { camera: AlignedCamera, time: f32 }, src/ray_tracer/vulkan.rs:113-118
 *    (68 B).  `time` is the RNG seed input (vulkan.rs:418-421 stamps unix_secs % 1000). */
typedef struct rvcp_push_constant {
    rvcp_camera_t camera;
    float time;
} rvcp_push_constant_t;

/* == AlignedMaterial, src/ray_tracer/scene/material.rs:20-28 (32 B, std140 array stride).
 *    ty: 0 Lambertian, 1 Metal, 2 Dielectric, 3 Light (material.rs:4-10). */
typedef struct rvcp_material {
    float albedo[3];        /* Le for lights */
    uint32_t ty;
    float fuzz;
    float refraction_ratio;
    uint32_t _padding[2];
} rvcp_material_t;

/* == AlignedVertex, src/ray_tracer/scene/mesh.rs:13-18 (32 B). */
typedef struct rvcp_vertex {
    float position[4];
    float normal[4];
} rvcp_vertex_t;

/* == AlignedFace, src/ray_tracer/scene/mesh.rs:37-42 (16 B). */
typedef struct rvcp_face {
    uint32_t vertices[3];
    uint32_t material_id;
} rvcp_face_t;

/* == AlignedSphere, src/ray_tracer/scene/sphere.rs:10-17 (32 B).  Traced by integrator
 *    RVCP_INTEGRATOR_LEGACY (ray_tracer.comp:300-321); the games101 shader never reads
 *    spheres. */
typedef struct rvcp_sphere {
    float center[3];
    float radius;
    uint32_t material_id;
    uint32_t _padding[3];
} rvcp_sphere_t;

/* == CameraData push constant of the Mandelbrot operator, src/mandelbrot/shader.rs:9-12 /
 *    assets/shaders/mandelbrot.comp:5-8 (vec2 position @0, float scale @8; 12 B). */
typedef struct rvcp_mandelbrot_push {
    float position[2];
    float scale;
} rvcp_mandelbrot_push_t;

/* == the 6 x u32 LengthBuffer, vulkan.rs:481-500 / ray_tracer_games101_branch.comp:58-65. */
typedef struct rvcp_lengths {
    uint32_t materials_len;
    uint32_t spheres_len;
    uint32_t vertices_len;
    uint32_t faces_len;
    uint32_t luminous_sphere_id_len;
    uint32_t luminous_face_id_len;
} rvcp_lengths_t;

/* ---------------------------------------------------------------------------------------
 * Configuration: the shader's compile-time #defines become runtime parameters with the
 * same defaults (ray_tracer_games101_branch.comp:5-13).
 * ------------------------------------------------------------------------------------- */
enum {
    /* ray_trace_games101 of ray_tracer_games101_branch.comp: the shader src/ray_tracer
     * dispatches (shader.rs:12).  Triangles only; area-light NEE; gamma 0.6 on store. */
    RVCP_INTEGRATOR_GAMES101 = 0,
    /* ray_trace of ray_tracer.comp (compiled by src/ray_tracer_deprecated/shader.rs:12):
     * spheres then triangles, Lambertian / metal / dielectric scattering, no NEE, no gamma
     * (ray_tracer.comp:618-694, :802-822).  Its #define defaults (ray_tracer.comp:5-13) come
     * from rvcp_config_default_for(RVCP_INTEGRATOR_LEGACY, ...); attenuation_stop_eps and
     * lum_id_std140_quirk are unused (the black-path test uses eps, :672). */
    RVCP_INTEGRATOR_LEGACY = 1,
};

enum {
    RVCP_ACCEL_NONE = 0,              /* brute-force scan, as the shader (parity) */
    RVCP_ACCEL_BVH = 1,               /* opt-in BVH (README.md:28-32 TODO "BVH") */
};

enum {
    RVCP_SPECIALIZE_AUTO = 0,
    RVCP_SPECIALIZE_OFF = 1,
};

enum {
    RVCP_UNORM_DRIVER = 0,            /* the reference driver's 12-bit fixed-point conversion */
    RVCP_UNORM_NEAREST = 1,           /* round-to-nearest */
};

typedef struct rvcp_config {
    int32_t device;                   /* HIP device ordinal */
    int32_t integrator;               /* RVCP_INTEGRATOR_* */
    uint32_t spp;                     /* SPP (:8) = 20 */
    uint32_t max_bounces;             /* MAX_BOUNCES (:9) = 15 */
    float attenuation_stop_eps;       /* ATTENUATION_STOP_EPS (:10) = 0.05 */
    float ray_t_min;                  /* RAY_T_MIN (:11) = 0.01 */
    float ray_t_max;                  /* RAY_T_MAX (:12) = 10000 */
    float rr_probability;             /* RR_PROBABILITY (:13) = 0.8 */
    float eps;                        /* EPS (:5) = 0.001 */
    /* 1 (default) reproduces what the reference GPU reads from the std140 `uint v[100]`
     * LuminousFaceIdBuffer that the host fills with tightly packed u32s
     * (ray_tracer_games101_branch.comp:109-111 vs vulkan.rs:473-478): element i is
     * ids[4*i] when 4*i < n_ids, else 0.  0 = the intended packed semantics. */
    int32_t lum_id_std140_quirk;
    /* Kernel schedule, for A/B measurement only: 0 = automatic (3; 6 for large frames with the
     * generic scan; 10 for meshes of 256+ faces on frames of 512 Ki samples or more, 5 on
     * smaller ones), 1 = one ray per lane per iteration, 2 = shadow + continuation ray per
     * lane per iteration, 3 = primary pre-pass + 2 over surface pixels (scalar-cache scan),
     * 4 = 3 with the scan staged through LDS tiles shared by the workgroup, 5 = 4 with one ray
     * per lane per iteration (shadow ray, then path ray: no empty ray slots), 6 = 3 compiled
     * for 6 waves per SIMD, 10 = 4 with the workgroup's rays pooled in LDS and scanned in
     * 64-ray passes (7, 8 and 9 are not schedules: the BVH wavefront form that held 9 was
     * measured 2.8x slower than the BVH path kernel and removed in round 4).  Every schedule
     * produces bit-identical frames. */
    int32_t kernel_variant;
    /* Acceleration structure: RVCP_ACCEL_NONE (default) scans every triangle like the
     * shader (bit-exact, the parity path).  RVCP_ACCEL_BVH (opt-in, games101 only) builds a
     * bounding-volume hierarchy at upload and tests only the triangles whose (slightly
     * enlarged) boxes the ray reaches, with the same exact triangle test and nearest-hit
     * rule; frames match the brute-force ones except where the exact test itself reports a
     * hit away from its triangle -- a ray almost parallel to the triangle's plane, or a sliver
     * or collinear triangle -- outside every box of that triangle.  The
     * box test of primary rays carries a relative slack for far cameras; tested: G-buffer
     * frames equal to the brute-force ones from 10, 100 and 1000 scene diagonals away, on
     * meshes and cameras with t_far x t_coef < 2^24 (renders: from cameras near the scene).  With
     * specialize = AUTO, a mesh whose leading faces (at most 64) are all large -- a room
     * around many small triangles, as C5 -- keeps those faces out of the BVH and tests them
     * first with the scene-specialised scan (the BVH hybrid; stats report
     * RVCP_VARIANT_SPECIALIZED). */
    int32_t accel;
    /* GPUs one context drives (0 or 1 = one).  With n_gpus = N > 1, rvcp_create opens devices
     * device, device+1, ... (mod the device count), rvcp_upload_scene uploads to all of them,
     * and rvcp_render deals the frame's 8-row stripes round-robin over them (stripe s -> GPU
     * s mod N), renders all shards concurrently and copies each shard's stripes into the frame
     * on `device` with one strided peer copy per shard (xGMI); the frame is bit-identical to
     * a 1-GPU render.  The single-process form of SURVEY.md §8(e); one process per GPU with
     * rvcp_render_shard_async + an RCCL gather (bench.py) is the other. */
    int32_t n_gpus;
    /* Float -> UNORM8 conversion of the stored colour (imageStore to the R8G8B8A8/B8G8R8A8
     * UNORM image, ray_tracer_games101_branch.comp:500, ray_tracer.comp:822,
     * mandelbrot.comp:33).  RVCP_UNORM_DRIVER (0, default): the conversion the reference's
     * driver performed, measured on its own render Notes/README/fractal.png (every one of its
     * 1,048,576 pixels reproduced): u8 = (floor(4096 x) * 255 + 2048) >> 12.
     * RVCP_UNORM_NEAREST (1): round-to-nearest, u8 = floor(255 x + 1/2). */
    int32_t unorm_rule;
    /* Scene-specialised scan: RVCP_SPECIALIZE_AUTO (0, default) compiles, at
     * rvcp_upload_scene, path kernels whose triangle scan is written out for the uploaded
     * scene (games101 integrator, brute force, at most 64 faces; hipRTC, ~1 s once per scene
     * and process) and uses them for schedules 3 and 6 when ray_t_min > 0 (and, with accel =
     * BVH, for the BVH hybrid's leading faces).  Frames are
     * bit-identical to the generic kernels; without hipRTC the generic kernels run.
     * RVCP_SPECIALIZE_OFF (1): always the generic kernels. */
    int32_t specialize;
    /* Persistent grid of one frame's path kernel, in waves per SIMD: 0 (default) = every
     * resident slot the kernel's occupancy allows; N > 0 caps it at N waves per SIMD (never
     * above the occupancy).  A pixel is a serial chain of SPP samples, so a frame ends with a
     * tail in which lanes whose pixels are done wait for the last chains; a caller that keeps
     * F > 1 frames in flight on F contexts can leave room for the next frame's waves so that
     * they start in that tail.  No effect on the frame's bits. */
    uint32_t grid_waves_per_simd;
} rvcp_config_t;

/* Per-render statistics (all optional). */
typedef struct rvcp_stats {
    double kernel_ms;                 /* device time of the render kernel(s), HIP events */
    uint64_t traversals;              /* scene traversals the reference algorithm performs
                                         (get_intersection_with_scene calls) */
    uint64_t traversals_executed;     /* traversals this kernel actually ran (primary hits
                                         are reused across a pixel's samples) */
    uint64_t samples;                 /* pixels * spp */
    uint32_t faces;                   /* F, triangles tested per traversal */
    int32_t kernel_variant;           /* the kernel schedule that ran (rvcp_config_t::
                                         kernel_variant resolved; 7 = BVH path kernel,
                                         8 = RVCP_INTEGRATOR_LEGACY kernel, 11 = the
                                         RVCP_MATERIALS_SCATTER kernel, 0 = none), plus
                                         RVCP_VARIANT_SPECIALIZED when the scene-specialised
                                         path kernel ran */
    uint64_t wave_iterations;         /* wave-level trace iterations; lane utilisation of the
                                         scan = traversals_executed / (64 * wave_iterations) */
    double main_kernel_ms;            /* device time of the dominant (path-tracing) kernel
                                         alone, HIP events on the launch stream; kernel_ms
                                         also covers the primary pre-pass and counter reset */
    double shader_clock_ghz;          /* the shader clock that kernel ran at: its waves'
                                         s_memtime ticks over their s_memrealtime (100 MHz)
                                         ticks, start to end, summed; 0 when not measured
                                         (schedules 1 / 2, trivial frames) */
} rvcp_stats_t;

#define RVCP_VARIANT_SPECIALIZED 16

/* ---------------------------------------------------------------------------------------
 * G-buffer and denoiser.  The reference has no counterpart: it stores the raw Monte-Carlo
 * frame (ray_tracer_games101_branch.comp:497-500) and its README lists only "BVH" and
 * "importance sampling" as TODO (README.md:28-32).  The filter is the edge-avoiding a-trous
 * wavelet transform of Dammertz, Sewtz, Hanika and Lensch (HPG 2010), guided by the primary
 * hit the pre-pass of the render already finds.
 * ------------------------------------------------------------------------------------- */
#define RVCP_GBUFFER_MISS      0xFFFFFFFFu   /* face: the primary ray hit nothing */
#define RVCP_GBUFFER_EMISSIVE  0x80000000u   /* material: bit 31 set when its ty is Light */

/* One pixel of rvcp_render_gbuffer_async: the primary hit as get_intersection_with_scene
 * (ray_tracer_games101_branch.comp:283-296) returns it for the pixel's sample_ray (:217-235).
 * A miss holds face = RVCP_GBUFFER_MISS and zeros elsewhere. */
typedef struct rvcp_gbuffer_texel {
    float position[3];      /* hit point, o + d t (:268) */
    uint32_t face;          /* face index, or RVCP_GBUFFER_MISS */
    float normal[3];        /* interpolated shading normal, turned to face the ray (:262-271) */
    uint32_t material;      /* face.material_id | RVCP_GBUFFER_EMISSIVE when its ty is 3 */
} rvcp_gbuffer_texel_t;

/* ---------------------------------------------------------------------------------------
 * Ray queries (rvcp_trace_rays_async; additions to 0.3.0, RVCP_ABI_VERSION
 * stays 2).  No counterpart in the reference, whose only rays are its own.
 * ------------------------------------------------------------------------------------- */
/* One ray of a query: points origin + t direction with t_min <= t <= t_max.  The direction
 * need not be normalised (t is in its units).  Every word must be finite: a ray with a NaN or an
 * infinity anywhere is reported as a miss and is not traced -- the one place where a query
 * decides before the scan does; it keeps such rays out of the tree.  A zero direction and
 * t_min > t_max go through the arithmetic like any other ray (and hit nothing). */
typedef struct rvcp_ray {
    float origin[3];
    float direction[3];
    float t_min;
    float t_max;
} rvcp_ray_t;

/* The nearest hit of one ray: what get_intersection_with_scene
 * (ray_tracer_games101_branch.comp:283-296) keeps for it -- every face tested with
 * is_intersect_with_face (:238-260), a hit accepted iff b1 >= 0, b2 >= 0, b1 + b2 <= 1 and
 * t_min <= t <= bt, with bt starting at the ray's own t_max and shrinking to each accepted t, so
 * that the later face wins at equal t.  face is numbered as rvcp_gbuffer_texel_t.face; t, b1, b2
 * are the winning test's own values (the hit point is v0 + b1 e1 + b2 e2 = origin + t direction
 * up to rounding).  A miss is face = -1 and zeros: the shader's t_max + 1 convention plays no
 * part, so t_max needs no 2^24 cap. */
typedef struct rvcp_ray_hit {
    int32_t face;           /* face index, or -1 */
    float t;
    float b1, b2;           /* barycentric weights of the face's second and third vertex */
} rvcp_ray_hit_t;

#define RVCP_RAYS_NEAREST 0   /* d_out: n rvcp_ray_hit_t */
#define RVCP_RAYS_ANY     1   /* d_out: n uint32_t, 1 = something lies in [t_min, t_max] */

#define RVCP_DENOISE_MAX_ITERATIONS 8

/* Parameters of rvcp_denoise_async (the filter's definition: DESIGN.md §4.9). */
typedef struct rvcp_denoise_params {
    uint32_t iterations;          /* a-trous passes, pass i with step 2^i; 1..8 */
    uint32_t normal_power_log2;   /* w_n = max(0, n_p . n_q) squared this many times; 0..8 */
    float sigma_color;            /* colour edge-stopping width at pass 0 (halved per pass),
                                     > 0; +inf switches the colour weight off */
    float sigma_plane;            /* plane-distance edge-stopping width, world units, > 0 */
} rvcp_denoise_params_t;

/* Temporal reprojection and accumulation.  No counterpart in the reference:
 * each of its frames starts from nothing. */
#define RVCP_TEMPORAL_MAX_HISTORY 65535u
#define RVCP_TEMPORAL_DENOISE     1u     /* rvcp_render_temporal flags: filter the displayed frame */

/* Parameters of rvcp_temporal_accumulate_async (the rule's definition: DESIGN.md §4.10). */
typedef struct rvcp_temporal_params {
    float alpha_min;        /* lower bound of the blend factor, 0..1 */
    uint32_t max_history;   /* cap of the per-pixel history length, 1..65535 */
    float sigma_plane;      /* a history tap is accepted within this distance of the pixel's
                               tangent plane, world units, > 0 */
    float normal_min;       /* ... and when n_p . n_q >= normal_min, -1..1 */
} rvcp_temporal_params_t;

/* The PREVIOUS frame's camera, ready to project a world point x into its pixel grid
 * (rvcp_temporal_view_from_push): with e = x - position and z = e . forward, the point lies at
 * pixel (e . right / z * k + W / 2 - 1/2, e . down / z * k + H / 2 - 1/2), pixel centres at the
 * integers -- the inverse of the shader's sample_ray (ray_tracer_games101_branch.comp:217-235). */
typedef struct rvcp_temporal_view {
    float position[3]; float k;         /* k = H / (2 tan(vfov/2 * PI/180)): pixels per unit slope */
    float right[3];    float _pad0;     /* normalize(forward x up) */
    float down[3];     float _pad1;     /* normalize(forward x right)  (sample_ray's v points down) */
    float forward[3];  float _pad2;     /* forward / (forward . forward) */
} rvcp_temporal_view_t;

/* Spatiotemporal variance-guided filtering (Schied et al., HPG 2017).  No
 * counterpart in the reference. */
#define RVCP_SVGF_MAX_ITERATIONS    8
#define RVCP_SVGF_MAX_SPATIAL_BELOW 16u
#define RVCP_SVGF_FEEDBACK          1u   /* rvcp_render_svgf flags: the colour history of the next
                                            frame is pass 0's output, not the raw accumulation */

/* Parameters of rvcp_svgf_accumulate_async (alpha_moments_min) and rvcp_svgf_filter_async (the
 * rest); the definitions: DESIGN.md §4.11. */
typedef struct rvcp_svgf_params {
    uint32_t iterations;          /* guided a-trous passes, pass i with step 2^i; 1..8 */
    uint32_t normal_power_log2;   /* w_n = max(0, n_p . n_q) squared this many times; 0..8 */
    float sigma_luminance;        /* luminance edge-stopping width in standard deviations of the
                                     pixel's own luminance, > 0; +inf switches the weight off */
    float sigma_plane;            /* plane-distance edge-stopping width, world units, > 0 */
    float epsilon;                /* added to sigma_luminance^2 x variance, > 0 */
    float alpha_moments_min;      /* lower bound of the moments' blend factor, 0..1 */
    uint32_t spatial_below;       /* a history shorter than this takes the 7 x 7 spatial variance
                                     estimate; 1..16, 1 = never */
    uint32_t _pad;                /* must be 0 */
} rvcp_svgf_params_t;

/* Temporal anti-aliasing: sub-pixel camera jitter and a clamped resolve.  No
 * counterpart in the reference: sample_ray (ray_tracer_games101_branch.comp:217-235) sends every
 * primary ray through the pixel centre. */
#define RVCP_TAA_JITTER_PERIOD 16u

/* Parameters of rvcp_taa_resolve_async (the rule's definition: DESIGN.md §4.13). */
typedef struct rvcp_taa_params {
    float alpha_min;        /* lower bound of the blend factor, 0..1 */
    uint32_t max_history;   /* cap of the per-pixel history length, 1..65535 */
    uint32_t clamp;         /* 1: the history is clamped into the colour box of the 3 x 3 current
                               pixels (not on the frame's border); 0: it is not */
    uint32_t _pad;          /* must be 0 */
} rvcp_taa_params_t;

/* Parameters of rvcp_taa_upsample_async (the rule's definition: DESIGN.md §4.14).  No
 * counterpart in the reference. */
typedef struct rvcp_taau_params {
    float max_weight;       /* cap of the per-pixel sample weight, finite, > 0 */
    float init_weight;      /* the weight of a pixel that starts a history, finite, > 0 */
    uint32_t clamp;         /* 1: the history is clamped into the colour box of the 3 x 3 traced
                               pixels (not where the traced pixel lies on its frame's border);
                               0: it is not */
    uint32_t _pad;          /* must be 0 */
} rvcp_taau_params_t;

/* Adaptive sampling: per-pixel sample counts.  No counterpart in the
 * reference: its shader gives every pixel the same SPP (ray_tracer_games101_branch.comp:8).
 * RVCP_SPP_MAP_MAX: the largest count a pixel of a map can get; the pre-pass clamps every word of
 * a map into 1..RVCP_SPP_MAP_MAX. */
#define RVCP_SPP_MAP_MAX 256u

/* Parameters of rvcp_spp_plan_async and rvcp_set_adaptive (the rule's definition: DESIGN.md
 * §4.18). */
typedef struct rvcp_adaptive_params {
    uint32_t spp_min;       /* every pixel gets at least this; 1..RVCP_SPP_MAP_MAX */
    uint32_t spp_max;       /* ... and at most this; spp_min..RVCP_SPP_MAP_MAX */
    float mean_spp;         /* the frame's budget, samples per pixel; spp_min..spp_max */
    float weight_cap;       /* priorities are cut off at this relative variance; finite, > 0 */
    float epsilon;          /* added to the squared luminance; finite, > 0 */
    uint32_t _pad;          /* must be 0 */
} rvcp_adaptive_params_t;

/* Layout checks: sizes/offsets the reference's Rust structs and std140/std430 blocks imply. */
#ifdef __cplusplus
#define RVCP_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define RVCP_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif
RVCP_STATIC_ASSERT(sizeof(rvcp_camera_t) == 64, "AlignedCamera is 64 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_camera_t, forward) == 32, "Camera.forward @32");
RVCP_STATIC_ASSERT(offsetof(rvcp_camera_t, t_near) == 44, "Camera.t_near @44");
RVCP_STATIC_ASSERT(offsetof(rvcp_camera_t, vertical_fov) == 52, "Camera.vertical_fov @52");
RVCP_STATIC_ASSERT(sizeof(rvcp_push_constant_t) == 68, "PushConstant is 68 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_push_constant_t, time) == 64, "PushConstant.time @64");
RVCP_STATIC_ASSERT(sizeof(rvcp_material_t) == 32, "AlignedMaterial is 32 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_material_t, ty) == 12, "Material.ty @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_material_t, refraction_ratio) == 20, "Material.ior @20");
RVCP_STATIC_ASSERT(sizeof(rvcp_vertex_t) == 32, "AlignedVertex is 32 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_vertex_t, normal) == 16, "Vertex.normal @16");
RVCP_STATIC_ASSERT(sizeof(rvcp_face_t) == 16, "AlignedFace is 16 B");
RVCP_STATIC_ASSERT(sizeof(rvcp_sphere_t) == 32, "AlignedSphere is 32 B");
RVCP_STATIC_ASSERT(sizeof(rvcp_lengths_t) == 24, "LengthBuffer is 24 B");
RVCP_STATIC_ASSERT(sizeof(rvcp_mandelbrot_push_t) == 12, "Mandelbrot CameraData is 12 B");
RVCP_STATIC_ASSERT(sizeof(rvcp_gbuffer_texel_t) == 32, "G-buffer texel is 32 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_gbuffer_texel_t, face) == 12, "GBuffer.face @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_gbuffer_texel_t, normal) == 16, "GBuffer.normal @16");
RVCP_STATIC_ASSERT(offsetof(rvcp_gbuffer_texel_t, material) == 28, "GBuffer.material @28");
RVCP_STATIC_ASSERT(sizeof(rvcp_ray_t) == 32, "a ray is 32 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_t, direction) == 12, "Ray.direction @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_t, t_min) == 24, "Ray.t_min @24");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_t, t_max) == 28, "Ray.t_max @28");
RVCP_STATIC_ASSERT(sizeof(rvcp_ray_hit_t) == 16, "a ray hit is 16 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_hit_t, t) == 4, "RayHit.t @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_hit_t, b1) == 8, "RayHit.b1 @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_ray_hit_t, b2) == 12, "RayHit.b2 @12");
RVCP_STATIC_ASSERT(sizeof(rvcp_denoise_params_t) == 16, "denoise params are 16 B");
RVCP_STATIC_ASSERT(sizeof(rvcp_temporal_params_t) == 16, "temporal params are 16 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_params_t, max_history) == 4, "TemporalParams.max_history @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_params_t, sigma_plane) == 8, "TemporalParams.sigma_plane @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_params_t, normal_min) == 12, "TemporalParams.normal_min @12");
RVCP_STATIC_ASSERT(sizeof(rvcp_temporal_view_t) == 64, "temporal view is 64 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_view_t, k) == 12, "TemporalView.k @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_view_t, right) == 16, "TemporalView.right @16");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_view_t, down) == 32, "TemporalView.down @32");
RVCP_STATIC_ASSERT(offsetof(rvcp_temporal_view_t, forward) == 48, "TemporalView.forward @48");
RVCP_STATIC_ASSERT(sizeof(rvcp_svgf_params_t) == 32, "SVGF params are 32 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, normal_power_log2) == 4, "SvgfParams.normal_power_log2 @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, sigma_luminance) == 8, "SvgfParams.sigma_luminance @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, sigma_plane) == 12, "SvgfParams.sigma_plane @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, epsilon) == 16, "SvgfParams.epsilon @16");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, alpha_moments_min) == 20, "SvgfParams.alpha_moments_min @20");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, spatial_below) == 24, "SvgfParams.spatial_below @24");
RVCP_STATIC_ASSERT(offsetof(rvcp_svgf_params_t, _pad) == 28, "SvgfParams._pad @28");
RVCP_STATIC_ASSERT(sizeof(rvcp_taa_params_t) == 16, "TAA params are 16 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_taa_params_t, max_history) == 4, "TaaParams.max_history @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_taa_params_t, clamp) == 8, "TaaParams.clamp @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_taa_params_t, _pad) == 12, "TaaParams._pad @12");
RVCP_STATIC_ASSERT(sizeof(rvcp_taau_params_t) == 16, "TAA upsampling params are 16 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_taau_params_t, init_weight) == 4, "TaauParams.init_weight @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_taau_params_t, clamp) == 8, "TaauParams.clamp @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_taau_params_t, _pad) == 12, "TaauParams._pad @12");
RVCP_STATIC_ASSERT(sizeof(rvcp_adaptive_params_t) == 24, "adaptive params are 24 B");
RVCP_STATIC_ASSERT(offsetof(rvcp_adaptive_params_t, spp_max) == 4, "AdaptiveParams.spp_max @4");
RVCP_STATIC_ASSERT(offsetof(rvcp_adaptive_params_t, mean_spp) == 8, "AdaptiveParams.mean_spp @8");
RVCP_STATIC_ASSERT(offsetof(rvcp_adaptive_params_t, weight_cap) == 12, "AdaptiveParams.weight_cap @12");
RVCP_STATIC_ASSERT(offsetof(rvcp_adaptive_params_t, epsilon) == 16, "AdaptiveParams.epsilon @16");
RVCP_STATIC_ASSERT(offsetof(rvcp_adaptive_params_t, _pad) == 20, "AdaptiveParams._pad @20");

typedef struct rvcp_ctx rvcp_ctx_t;

/* Error codes */
#define RVCP_OK               0
#define RVCP_E_INVALID      (-1)   /* bad argument */
#define RVCP_E_HIP          (-2)   /* HIP runtime error */
#define RVCP_E_NO_SCENE     (-3)   /* render before upload */
#define RVCP_E_UNSUPPORTED  (-4)
#define RVCP_E_NOMEM        (-5)   /* host or device allocation failed */
#define RVCP_E_INTERNAL     (-6)   /* unexpected internal error (caught at the ABI boundary) */
#define RVCP_E_TIMEOUT      (-7)   /* a collective did not complete within the deadline
                                    * (rvcp_rccl_set_timeout): a peer rank is missing or failed;
                                    * the context's own communicator has been aborted */
#define RVCP_E_BUSY         (-8)   /* rvcp_rccl_init refused: the context's previous creation
                                    * timed out and its worker is still blocked inside RCCL */

/* ABI revision of this header, returned by rvcp_abi_version().  2 (round 6): rvcp_stats_t grew
 * from 56 to 64 bytes (shader_clock_ghz), RVCP_E_TIMEOUT / RVCP_E_BUSY, rvcp_abi_version and the
 * code-cache entry points.  A caller compiled against another revision must not pass its
 * rvcp_stats_t ("ABI revisions"). */
#define RVCP_ABI_VERSION 2

/* ---------------------------------------------------------------------------------------
 * Entry points
 * ------------------------------------------------------------------------------------- */

/* Library version string. */
const char *rvcp_version(void);

/* RVCP_ABI_VERSION of the header the library was built with: a caller checks it against its
 * own before passing structs (rvcp_stats_t changed size between revisions 1 and 2). */
uint32_t rvcp_abi_version(void);

/* On-disk cache of the scene-specialised code objects: rvcp_upload_scene
 * compiles a module per scene with hipRTC (~0.7 s); with a cache directory the code object is
 * stored under a key that covers the generated source, the kernel source, the compile options
 * and the hipRTC version, and a later process that uploads the same scene loads it instead.
 * An entry is checked (header, key, length, checksum) before it is loaded; a damaged or
 * foreign entry is recompiled and rewritten, never trusted.  The checksum detects damage, not
 * tampering: the directory is trusted like the user's own files (as any JIT cache is), so it
 * must not be writable by others (the library creates it 0700).  The reference has no counterpart
 * (its SPIR-V is compiled into the binary, src/ray_tracer/shader.rs:9-14).
 * dir: the directory (created if missing); NULL or "" disables the cache.  Default:
 * $XDG_CACHE_HOME/rvcp-mi355x, else $HOME/.cache/rvcp-mi355x (the only environment the product
 * library reads).  Process-wide. */
int rvcp_set_code_cache_dir(const char *dir);

/* Counters of the on-disk cache since the process started: out[0] modules loaded from disk,
 * out[1] modules compiled (and stored), out[2] entries rejected (damaged / foreign / unloadable)
 * and recompiled. */
int rvcp_code_cache_counts(uint64_t out[3]);

/* Fill `cfg` with the reference's #define defaults.  Replaces nothing (the reference bakes
 * them into the SPIR-V at `vulkano_shaders::shader!`, src/ray_tracer/shader.rs:9-14). */
int rvcp_config_default(rvcp_config_t *cfg);

/* Same, for integrator `integrator` (RVCP_INTEGRATOR_*): the #defines of the shader that
 * integrator restates (ray_tracer_games101_branch.comp:5-13 or ray_tracer.comp:5-13).
 * RVCP_E_UNSUPPORTED for an unknown integrator. */
int rvcp_config_default_for(int32_t integrator, rvcp_config_t *cfg);

/* Create a context on cfg->device.  Replaces pipeline creation:
 * `Vk::create_compute_pipeline(device, ray_tracer_shader::load(device))`,
 * src/ray_tracer/vulkan.rs:576-603 (called at :239-242). */
int rvcp_create(const rvcp_config_t *cfg, rvcp_ctx_t **out_ctx);

/* Free the context and all device memory it owns. */
int rvcp_destroy(rvcp_ctx_t *ctx);

/* Last error message for `ctx` ("" if none).  ctx may be NULL (global create errors). */
const char *rvcp_last_error(const rvcp_ctx_t *ctx);

/* Upload a scene.  Replaces `Vk::create_descriptor_set_0s`, src/ray_tracer/vulkan.rs:454-574
 * (bindings 1 LengthBuffer, 2 MaterialBuffer, 4 VertexBuffer, 5 FaceBuffer,
 * 7 LuminousFaceIdBuffer).  `lum_face_ids` are the packed u32 ids the host computes at
 * vulkan.rs:473-478; the std140 quirk is applied inside.  Spheres (binding 3) are traced by
 * RVCP_INTEGRATOR_LEGACY and ignored by games101; luminous sphere ids (binding 6) are read
 * by neither integrator's dispatched path and may be NULL/0.  Face vertex indices and
 * material ids are validated (the reference does not bound-check; out-of-range ids are an
 * error). */
int rvcp_upload_scene(rvcp_ctx_t *ctx,
                      const rvcp_material_t *materials, uint32_t n_materials,
                      const rvcp_vertex_t *vertices, uint32_t n_vertices,
                      const rvcp_face_t *faces, uint32_t n_faces,
                      const rvcp_sphere_t *spheres, uint32_t n_spheres,
                      const uint32_t *lum_face_ids, uint32_t n_lum_face_ids,
                      const uint32_t *lum_sphere_ids, uint32_t n_lum_sphere_ids);

/* Load a binary scene file (.rvcpscn: "RVCPSCN1" header, rvcp_lengths_t, rvcp_camera_t,
 * then the upload arrays in the layouts above; format in scene_io.py) and upload it as
 * rvcp_upload_scene would.  The camera stored in the file is copied to *out_camera when
 * non-NULL.  Replaces the reference's compiled-in scene (`Scene::default`,
 * src/ray_tracer/scene/mod.rs:21) as the way to feed large meshes.
 * RVCP_E_INVALID for an unreadable, truncated or malformed file. */
int rvcp_upload_scene_file(rvcp_ctx_t *ctx, const char *path, rvcp_camera_t *out_camera);

/* Render one full frame synchronously into host memory.  Replaces the per-frame
 * `push_constants(...)` + `dispatch([W/8, H/8, 1])` + present of vulkan.rs:406-452 and
 * :298-404.  out_rgba8: W*H*4 bytes, row-major, logical RGBA (the reference's swapchain was
 * B8G8R8A8_UNORM, records/swapchain_image.txt:8), alpha 255.  out_linear_rgb (optional):
 * W*H*3 floats, the pre-clamp, pre-gamma `color` of ray_tracer_games101_branch.comp:497
 * (ray_tracer.comp:819 for RVCP_INTEGRATOR_LEGACY, whose RGBA8 store has no gamma).
 * Unlike the reference, W and H need not be multiples of 8 (every pixel is rendered). */
int rvcp_render(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                uint32_t width, uint32_t height,
                uint8_t *out_rgba8, float *out_linear_rgb, rvcp_stats_t *stats);

/* The reference's second compute operator, assets/shaders/mandelbrot.comp (dispatched by
 * src/mandelbrot/vulkan.rs:380-400 with CameraData {position, scale}; defaults [0, 0] and 1.0,
 * src/mandelbrot/config.rs:11-12).  Writes the W x H grey RGBA8 frame (escape time i,
 * UNORM8, alpha 255) and optionally the float i per pixel.  Synchronous, like rvcp_render;
 * needs no scene.  stats (optional) gets kernel_ms only. */
int rvcp_mandelbrot(rvcp_ctx_t *ctx, const rvcp_mandelbrot_push_t *push,
                    uint32_t width, uint32_t height,
                    uint8_t *out_rgba8, float *out_value, rvcp_stats_t *stats);

/* Asynchronous shard render into device memory, for multi-GPU frame assembly.
 * The frame is cut into 8-row stripes (the reference's 8x8 workgroup rows); stripe s is
 * rendered by shard (s % shard_count).  This call renders the stripes of `shard_index`
 * and packs them contiguously, in increasing stripe order, into d_rgba8
 * (rvcp_shard_rows(H, idx, count) * W * 4 bytes) and optionally d_linear_rgb (rows*W*3
 * floats).  Pixel values are bit-identical to a single-GPU render of the whole frame.
 * Enqueued on `stream`; stats->kernel_ms/traversals are filled by rvcp_sync_stats(). */
int rvcp_render_shard_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                            uint32_t width, uint32_t height,
                            uint32_t shard_index, uint32_t shard_count,
                            void *d_rgba8, void *d_linear_rgb, void *stream);

/* A batch of n_frames consecutive frames of one shard (frame k rendered with pushes[k]: its
 * camera and its time seed), enqueued as one unit on `stream`.  The swapchain loop of
 * vulkan.rs:367-369, 392-401 keeps one frame per swapchain image in flight; here the frames
 * of a batch share one surface list and one persistent path kernel, so lanes whose pixels of
 * frame k are done take pixels of frame k+1 while the last sample chains of frame k finish
 *  -- frames in flight at lane granularity instead of wave granularity.
 * Layout: frame k's packed shard rows start at pixel k * S of d_rgba8 (and of d_linear_rgb,
 * 3 floats per pixel, optional), S = rvcp_shard_rows(height, 0, shard_count) * width, the
 * largest shard's pixels (for a smaller shard the rows after its own are padding and hold
 * unspecified values); with shard_count = 1, S = W*H and the frames are simply consecutive.
 * Every frame is bit-identical to rvcp_render_shard_async with the same push.  One pending
 * batch per context; rvcp_sync_stats covers the whole batch (samples = n_frames x shard
 * pixels x spp).  Integrator mode 2 (RVCP_INTEGRATOR_LEGACY) has no pre-pass: its one kernel
 * queues the batch's pixels frame after frame, reading each frame's camera and time from a
 * table the call uploads.  Needs a one-GPU context and, for games101, a pre-pass schedule (the
 * automatic ones: 3-6, 10, the BVH path kernel); schedules 1 and 2 return
 * RVCP_E_UNSUPPORTED unless n_frames = 1. */
int rvcp_render_frames_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *pushes,
                             uint32_t n_frames, uint32_t width, uint32_t height,
                             uint32_t shard_index, uint32_t shard_count,
                             void *d_rgba8, void *d_linear_rgb, void *stream);

/* Wait for the last async render of ctx and fetch its statistics.  It waits for the render
 * only: a gather enqueued behind it (rvcp_gather_frame_async) needs rvcp_gather_wait before
 * rank 0's assembled frame may be read. */
int rvcp_sync_stats(rvcp_ctx_t *ctx, rvcp_stats_t *stats);

/* The asynchronous pair of SURVEY.md §8(b) (the reference's per-image fences,
 * vulkan.rs:367-369, 392-401): enqueue one full frame into DEVICE memory on `stream` (NULL:
 * the context's own stream) and return; rvcp_wait blocks until it is done and fills stats.
 * d_rgba8: W*H*4 bytes, d_linear_rgb (optional): W*H*3 floats, as rvcp_render.  Equivalent to
 * rvcp_render_shard_async(..., 0, 1, ...) / rvcp_sync_stats.  One GPU: a context with
 * n_gpus > 1 returns RVCP_E_UNSUPPORTED (use rvcp_render). */
int rvcp_render_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                      uint32_t width, uint32_t height,
                      void *d_rgba8, void *d_linear_rgb, void *stream);
int rvcp_wait(rvcp_ctx_t *ctx, rvcp_stats_t *stats);

/* Rows of an H-row frame owned by shard `shard_index` of `shard_count`. */
uint32_t rvcp_shard_rows(uint32_t height, uint32_t shard_index, uint32_t shard_count);

/* Assemble a frame on the device from gathered shard buffers.  d_gathered holds
 * shard_count slots of `slot_rows` rows (slot_rows >= max shard rows) each, shard k's
 * packed stripes at slot k.  Writes the W x H RGBA8 frame to d_frame.  Enqueued on stream. */
int rvcp_assemble_frame_async(rvcp_ctx_t *ctx, const void *d_gathered, uint32_t slot_rows,
                              uint32_t width, uint32_t height, uint32_t shard_count,
                              void *d_frame, void *stream);

/* ---------------------------------------------------------------------------------------
 * One process per GPU: every rank renders its stripes with
 * rvcp_render_shard_async(ctx, ..., rank, world, d_shard, ...) into a shard buffer of
 * rvcp_shard_rows(H, 0, world) rows (shard 0 has the most rows; shorter shards send padding),
 * then rvcp_gather_frame_async gathers the shards to rank 0 with one RCCL ncclGather over
 * xGMI and assembles the frame there on the device.  The reference is single-device
 * (src/ray_tracer/vulkan.rs:145-193 picks one physical device); this replaces nothing in it
 * and adds the multi-GPU form north_star asks for.  RCCL is loaded at run time
 * (librccl.so.1: the copy the process already holds, e.g. PyTorch-ROCm's, else the system
 * one); without it these return RVCP_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
#define RVCP_RCCL_ID_BYTES 128     /* sizeof(ncclUniqueId) */

/* Rank 0: create the communicator id (ncclGetUniqueId) to hand to every rank by any
 * out-of-band channel (MPI, a TCP store, torch.distributed's broadcast). */
int rvcp_rccl_unique_id(uint8_t out_id[RVCP_RCCL_ID_BYTES]);

/* Every rank, collectively: create ctx's communicator (non-blocking ncclCommInitRankConfig on
 * ctx's device, polled with ncclCommGetAsyncError).  Returns once all `world` ranks have
 * joined, or RVCP_E_TIMEOUT when they have not within the context's deadline.  The creation
 * runs on a worker thread, because RCCL's "non-blocking" creation call itself does not return
 * while a peer is absent: on a timeout the worker is left behind (it aborts the half-made
 * communicator if RCCL ever returns), the message counts such workers in the process, and the
 * context refuses a further rvcp_rccl_init with RVCP_E_BUSY while its worker is still blocked --
 * at most one blocked worker per context; the context stays usable for single-GPU renders (and
 * rvcp_rccl_attach).  Destroyed with the context.  The reference has no counterpart (single device); its own
 * recover-not-hang path is the swapchain's OutOfDate -> recreate (src/ray_tracer/vulkan.rs:
 * 355-364). */
int rvcp_rccl_init(rvcp_ctx_t *ctx, const uint8_t id[RVCP_RCCL_ID_BYTES], uint32_t world,
                   uint32_t rank);

/* Deadline of rvcp_rccl_init and rvcp_gather_wait (and of the wait for a pending gather in
 * rvcp_destroy), in milliseconds; 0 = wait forever.  Default 60000.  It must exceed the
 * render time of the frames a gather waits behind. */
int rvcp_rccl_set_timeout(rvcp_ctx_t *ctx, uint32_t timeout_ms);

/* Use the caller's existing communicator (an ncclComm_t over ctx's device, rank `rank` of
 * `world`) instead; the caller keeps ownership (and is the one to abort it).  A non-blocking
 * communicator (ncclConfig_t.blocking = 0) is supported: a gather that returns ncclInProgress
 * is polled until it is on the stream, bounded by the deadline. */
int rvcp_rccl_attach(rvcp_ctx_t *ctx, void *nccl_comm, uint32_t world, uint32_t rank);

/* Every rank, collectively, after its rvcp_render_shard_async on the same stream: gather the
 * shards to rank 0 (ncclGather, root 0, shard k at slot k of d_gathered) and, on rank 0,
 * assemble the W x H RGBA8 frame into d_frame.  d_shard_rgba8: rvcp_shard_rows(H, 0, world)
 * * W * 4 bytes on every rank; d_gathered (world times that) and d_frame (W*H*4 bytes) are
 * needed on rank 0 only (NULL elsewhere).  Enqueued on `stream`, behind the caller's own
 * ordering; with stream = NULL on ctx's gather stream (highest priority), after the
 * preceding render by an event, and the next render on ctx waits for the gather by an event,
 * so the render stream is free for the next frame meanwhile.  The frame is bit-identical to
 * a single-GPU render.  The preceding render on ctx must have been
 * shard_index = rank, shard_count = world of the same W x H frame (else RVCP_E_INVALID). */
int rvcp_gather_frame_async(rvcp_ctx_t *ctx, const void *d_shard_rgba8, uint32_t width,
                            uint32_t height, void *d_gathered, void *d_frame, void *stream);

/* Wait for ctx's last rvcp_gather_frame_async and report its device time (ncclGather plus, on
 * rank 0, the assembly) in *gather_ms and, if frame_ms is not NULL, the time from the start of
 * the preceding render to the end of the gather in *frame_ms (HIP events on the gather's
 * stream).  RVCP_E_INVALID when no gather was enqueued since the last call.  The wait polls
 * against the context's deadline (rvcp_rccl_set_timeout): when the gather has not finished by
 * then -- a peer rank never entered it -- or RCCL reports an asynchronous error, the
 * context's communicator is aborted (ncclCommAbort; its kernels exit) and RVCP_E_TIMEOUT
 * (resp. RVCP_E_HIP) is returned; rvcp_rccl_init may then build a new one.  An attached
 * communicator is not aborted (it is the caller's) but dropped.  When the gather's stream has
 * not drained (always the case for an attached communicator whose peer never comes), later
 * renders on ctx no longer wait for that gather, later gathers return RVCP_E_TIMEOUT until a
 * new communicator is initialised or attached (they then run on a fresh gather stream), and
 * rvcp_destroy waits for the stuck gather at most min(deadline, 10 s): past that it frees the
 * host side, leaks the context's device memory and streams (a hipFree would wait for the stuck
 * collective: HIP synchronises the device) and returns RVCP_E_TIMEOUT, with the message in
 * rvcp_last_error(NULL).
 * rvcp_sync_stats / rvcp_wait wait for the render only: rank 0's assembled frame (d_frame)
 * is complete after this call, not after theirs. */
int rvcp_gather_wait(rvcp_ctx_t *ctx, float *gather_ms, float *frame_ms);

/* ---------------------------------------------------------------------------------------
 * G-buffer + edge-avoiding a-trous denoiser (opt-in; no other entry point changes).  No
 * counterpart in the reference (see the structs above).
 * ------------------------------------------------------------------------------------- */

/* Enqueue the G-buffer of one frame on `stream`: W*H rvcp_gbuffer_texel_t, row-major, into
 * device memory.  One lane per pixel traces the primary ray with the render's own scan (the
 * BVH with accel = RVCP_ACCEL_BVH), so each texel is the hit the render's pre-pass finds and
 * the shader's get_intersection_with_scene returns, bit for bit.  Ordered on `stream` like
 * the other async calls; it is not the context's pending frame (nothing to wait for but the
 * stream) and touches no statistics.  games101 integrator on a one-GPU context only:
 * RVCP_INTEGRATOR_LEGACY and n_gpus > 1 return RVCP_E_UNSUPPORTED. */
int rvcp_render_gbuffer_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                              uint32_t width, uint32_t height, void *d_gbuffer, void *stream);

/* The default filter parameters (the best row on average of the sweep of
 * tools/denoise_sweep.py over the Cornell box at SPP 1, 4 and 10).  Needs no device. */
int rvcp_denoise_params_default(rvcp_denoise_params_t *params);

/* Enqueue the filter on `stream`: d_linear_rgb_in (W*H*3 floats, e.g. the linear output of
 * rvcp_render_async) filtered under d_gbuffer (W*H texels) into d_linear_rgb_out (W*H*3
 * floats, must not overlap the input) and, when d_rgba8_out is not NULL, pow(clamp(c), 0.6) of
 * the result as RGBA8 under the context's unorm_rule (W*H*4 bytes, alpha 255), exactly as the
 * render stores its own frame.  A pixel is filterable when its texel is a hit on a
 * non-emissive material; other pixels pass through unchanged and feed no neighbour.  All
 * weights are single correctly rounded f32 operations in a fixed order, so
 * the result is reproducible bit for bit.  params = NULL: the defaults.  Needs no scene.
 * The passes between the first and the last go through buffers the context owns.  A render
 * pending on the context is not an error: the filter is ordered behind it.
 * RVCP_E_INVALID: NULL / zero arguments, overlapping input and output, iterations outside
 * 1..RVCP_DENOISE_MAX_ITERATIONS, normal_power_log2 > 8, a sigma that is not > 0. */
int rvcp_denoise_async(rvcp_ctx_t *ctx, const void *d_linear_rgb_in, const void *d_gbuffer,
                       uint32_t width, uint32_t height, const rvcp_denoise_params_t *params,
                       void *d_linear_rgb_out, void *d_rgba8_out, void *stream);

/* Wait for the context's last rvcp_denoise_async; *denoise_ms (optional) gets its device
 * time, first pass to the RGBA8 store (HIP events on its stream).  RVCP_E_INVALID when no
 * filter was enqueued since the last call. */
int rvcp_denoise_wait(rvcp_ctx_t *ctx, float *denoise_ms);

/* Render + G-buffer + filter of one frame, synchronously into host memory, on the context's
 * stream and in buffers the context owns: out_rgba8 (W*H*4 bytes) and out_linear_rgb
 * (optional, W*H*3 floats) are the filtered frame; stats (optional) are the render's,
 * *denoise_ms (optional) as rvcp_denoise_wait.  Restrictions of rvcp_render_gbuffer_async. */
int rvcp_render_denoised(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                         uint32_t width, uint32_t height, const rvcp_denoise_params_t *params,
                         uint8_t *out_rgba8, float *out_linear_rgb, rvcp_stats_t *stats,
                         float *denoise_ms);

/* ---------------------------------------------------------------------------------------
 * Ray queries: nearest hit and occlusion for rays the caller supplies (opt-in; no other entry
 * point changes).  Triangles only, as the G-buffer: spheres are not tested.
 * ------------------------------------------------------------------------------------- */

/* Enqueue a query on `stream`: n_rays rvcp_ray_t in device memory (16-byte aligned) traced
 * against the uploaded scene, one lane per ray, with the render's own tests -- the generic scan
 * over every face, or with accel = RVCP_ACCEL_BVH the hybrid's prefix faces and then the tree,
 * as rvcp_render_gbuffer_async -- so a result is the brute-force scan's, bit for bit (the
 * struct comments above define it; the tree's exactness is argued in DESIGN.md §4.6 and tested
 * on these very rays, §4.19).  mode RVCP_RAYS_NEAREST writes n_rays rvcp_ray_hit_t (16-byte
 * aligned) to d_out; RVCP_RAYS_ANY writes n_rays uint32_t (4-byte aligned), 1 exactly where
 * NEAREST would report a hit -- it may stop at the first accepted face, which only skips work
 * NEAREST does after it already holds a hit.  Ordered on `stream` (NULL: the context's) like the
 * other async calls, behind a render pending on the context (not an error) and behind the
 * context's previous query; it is not the context's pending frame and touches no statistics.
 * RVCP_E_INVALID: a NULL or zero argument, n_rays >= 2^31, another mode, a misaligned buffer.
 * RVCP_E_NO_SCENE before an upload.  RVCP_E_UNSUPPORTED: a RVCP_INTEGRATOR_LEGACY or n_gpus > 1 context. */
int rvcp_trace_rays_async(rvcp_ctx_t *ctx, const void *d_rays, uint32_t n_rays, uint32_t mode,
                          void *d_out, void *stream);

/* Wait for the context's last rvcp_trace_rays_async; *rays_ms (optional) gets its device time
 * (HIP events on its stream).  RVCP_E_INVALID when no query was enqueued since the last call. */
int rvcp_rays_wait(rvcp_ctx_t *ctx, float *rays_ms);

/* The same query from and into host memory, synchronously, on the context's stream and through
 * staging the context owns: out is n_rays rvcp_ray_hit_t or uint32_t by mode; *rays_ms
 * (optional) gets its device time.  It is ordered behind a pending rvcp_trace_rays_async and
 * leaves it pending: that query's rvcp_rays_wait still returns its own time. */
int rvcp_trace_rays(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, uint32_t n_rays, uint32_t mode,
                    void *out, float *rays_ms);

/* Enqueue on `stream` the W*H rays the pre-pass and the G-buffer trace, in pixel order
 * (row-major), as rvcp_ray_t into device memory (16-byte aligned): origin the camera, direction
 * normalised, [t_min, t_max] = [t_near, t_far] x t_coef (sample_ray, :217-235).  Tracing them
 * with RVCP_RAYS_NEAREST gives the G-buffer's face at every pixel.  Restrictions and checks of
 * rvcp_render_gbuffer_async (W*H < 2^31, t_far x t_coef < 2^24). */
int rvcp_primary_rays_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                            uint32_t height, void *d_rays, void *stream);

/* The nearest hit under pixel (x, y) of the W x H frame: that pixel's primary ray and a one-ray
 * RVCP_RAYS_NEAREST query, synchronously, in buffers the context owns (and, as
 * rvcp_trace_rays, without disturbing a pending rvcp_trace_rays_async).  RVCP_E_INVALID also for
 * x >= width or y >= height. */
int rvcp_pick(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width, uint32_t height,
              uint32_t x, uint32_t y, rvcp_ray_hit_t *out_hit);

/* ---------------------------------------------------------------------------------------
 * Path queries: the radiance along rays the caller supplies (opt-in; no other entry point
 * changes; additions to 0.3.0, RVCP_ABI_VERSION stays 2).  Triangles only, the
 * games101 integrator with the uniform bounce.  No new structs: rays are rvcp_ray_t, seeds are
 * float, a result is three float per ray, the layout of a linear frame.
 * ------------------------------------------------------------------------------------- */

/* Enqueue a query on `stream`: n_rays rvcp_ray_t (16-byte aligned) and n_rays float seeds
 * (4-byte aligned) in device memory -> n_rays * 3 floats of linear RGB (4-byte aligned); spp in
 * 1..RVCP_SPP_MAP_MAX.
 *
 * Result.  The result of ray i is what main (ray_tracer_games101_branch.comp:486-496) would leave
 * in `color` for a pixel whose sample_ray is ray i taken as given (the direction is used as it is
 * and is not normalised), whose srand result is seeds[i] (the rand() index starts at 0 and runs
 * on from sample to sample) and whose SPP is spp: color += ray_trace(ray) / spp, spp times, in
 * that order, with the context's max_bounces, rr_probability, eps, attenuation_stop_eps,
 * ray_t_min, ray_t_max and light-pick quirk -- bit for bit.  The record's [t_min, t_max] bounds
 * the first segment only; later segments use the configuration's range, as in the shader.
 * "Nothing accepted" is a miss and adds the shader's 0.1: that is the shader's own t > t_max test
 * (:424) for t_max < 2^24, where its t_max + 1 (:287) is still above t_max; a record with a
 * larger t_max is traced all the same, by the absent face.
 *
 * Rejected rays.  A ray is not traced, draws no random number and returns (0, 0, 0) when any of
 * its eight words is not finite, or when its seed is not in [0, 1) (a NaN seed is outside; srand
 * only ever returns a fract).  It does not disturb the other rays of the query.
 *
 * Ordered on `stream` (NULL: the context's) like the other async calls, behind a render pending
 * on the context (not an error) and behind the context's previous path query; one query is in
 * flight per context (a second enqueue before rvcp_paths_wait replaces what the wait reports).
 * It touches neither rvcp_stats_t nor the render's counters, and the ray queries not at all.
 *
 * RVCP_E_INVALID: a NULL or zero argument, n_rays >= 2^31, spp outside 1..RVCP_SPP_MAP_MAX, a
 * misaligned buffer, an output that overlaps an input.  RVCP_E_NO_SCENE before an upload.
 * RVCP_E_UNSUPPORTED: a RVCP_INTEGRATOR_LEGACY or n_gpus > 1 context, or one whose sampling mode
 * is RVCP_SAMPLING_COSINE (the query kernel holds the uniform bounce only).  An error leaves the
 * output untouched and nothing pending. */
int rvcp_trace_paths_async(rvcp_ctx_t *ctx, const void *d_rays, const void *d_seeds,
                           uint32_t n_rays, uint32_t spp, void *d_linear_rgb_out, void *stream);

/* Wait for the pending path query: *paths_ms (optional) gets its device time (HIP events on its
 * stream), *traversals (optional) the calls of get_intersection_with_scene it stands for, as the
 * reference makes them: a first hit that the kernel keeps and reuses counts once per sample.
 * RVCP_E_INVALID when no query was enqueued since the last call. */
int rvcp_paths_wait(rvcp_ctx_t *ctx, float *paths_ms, uint64_t *traversals);

/* The same from and to host memory, synchronously, on the context's stream and in staging the
 * context owns.  It is ordered behind a pending rvcp_trace_paths_async and leaves it pending:
 * that query's rvcp_paths_wait still returns its own time and traversals. */
int rvcp_trace_paths(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, const float *seeds, uint32_t n_rays,
                     uint32_t spp, float *out_linear_rgb, float *paths_ms, uint64_t *traversals);

/* Enqueue on `stream` the W*H seeds main() gives the frame's pixels, srand(push->time, u, v)
 * (:153-155, :488-489), row-major, as float into device memory (4-byte aligned): the companion of
 * rvcp_primary_rays_async, with its checks.  The frame's primary rays and these seeds through
 * rvcp_trace_paths_async with the context's spp give rvcp_render_async's linear frame. */
int rvcp_primary_seeds_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                             uint32_t height, void *d_seeds, void *stream);

/* ---------------------------------------------------------------------------------------
 * Temporal reprojection and accumulation of frames across calls (opt-in; no other entry point
 * changes).  No counterpart in the reference.
 * ------------------------------------------------------------------------------------- */

/* The default parameters: alpha_min 0.05, max_history 32, sigma_plane 0.1, normal_min 0.9.
 * Needs no device. */
int rvcp_temporal_params_default(rvcp_temporal_params_t *params);

/* The projection of `push`'s camera for a width x height frame, computed in double and rounded
 * once to float (PI = 3.1415926, the shader's constant).  Needs no device.  RVCP_E_INVALID:
 * NULL / zero arguments, or a camera whose forward is zero or parallel to up. */
int rvcp_temporal_view_from_push(const rvcp_push_constant_t *push, uint32_t width, uint32_t height,
                                 rvcp_temporal_view_t *out_view);

/* Enqueue one accumulation step on `stream`; stateless, every buffer is the caller's device
 * memory.  d_cur_linear (W*H*3 floats) and d_cur_gbuffer (W*H texels) are the current frame;
 * d_prev_linear, d_prev_gbuffer and d_prev_len (W*H uint32_t) the accumulated previous frame, its
 * G-buffer and its per-pixel history lengths -- all three NULL: no history, every filterable
 * pixel starts one.  `view` is the previous frame's camera (rvcp_temporal_view_from_push); NULL
 * means the camera did not move and pixel p continues the history of pixel p.  Written:
 * d_out_linear (W*H*3 floats), d_out_len (W*H uint32_t: 0 on a non-filterable pixel, which passes
 * through; 1 where a history starts) and, when d_rgba8_out is not NULL, pow(clamp(c), 0.6) of the
 * result as RGBA8 under the context's unorm_rule, exactly as the render stores its own frame.
 * All arithmetic is single correctly rounded f32 operations in a fixed order,
 * so the result is reproducible bit for bit.  params = NULL: the defaults.  Needs no scene.  A
 * render pending on the context is not an error: the step is ordered behind it, and behind the
 * context's previous step.
 * RVCP_E_INVALID: NULL / zero arguments, an output that overlaps an input or another output,
 * some but not all of d_prev_*, alpha_min outside 0..1, max_history outside 1..65535,
 * sigma_plane not > 0, normal_min outside -1..1 (a NaN is outside every range). */
int rvcp_temporal_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                                   const void *d_cur_linear, const void *d_cur_gbuffer,
                                   const void *d_prev_linear, const void *d_prev_gbuffer,
                                   const void *d_prev_len, uint32_t width, uint32_t height,
                                   const rvcp_temporal_params_t *params, void *d_out_linear,
                                   void *d_out_len, void *d_rgba8_out, void *stream);

/* Wait for the context's last rvcp_temporal_accumulate_async; *temporal_ms (optional) gets its
 * device time, kernel to the RGBA8 store (HIP events on its stream).  RVCP_E_INVALID when no
 * step was enqueued since the last call. */
int rvcp_temporal_wait(rvcp_ctx_t *ctx, float *temporal_ms);

/* Render + G-buffer + accumulation [+ filter] of one frame, synchronously into host memory, on
 * the context's stream and in buffers the context owns.  The context keeps the accumulated
 * frame, its history lengths and its G-buffer from call to call, with the camera they were
 * rendered from; the next call reprojects through that camera, or continues pixel by pixel when
 * the 64 camera bytes of `push` equal the previous call's.  The history is dropped (every
 * filterable pixel restarts at length 1) on the first call, when width or height change, on
 * rvcp_upload_scene / rvcp_upload_scene_file and on rvcp_temporal_reset.
 * flags & RVCP_TEMPORAL_DENOISE: the displayed frame is rvcp_denoise_async(dparams) of the
 * accumulated one; the history keeps the unfiltered accumulation.
 * out_rgba8 (W*H*4 bytes) and out_linear_rgb (optional, W*H*3 floats) are the displayed frame,
 * out_history_len (optional, W*H uint32_t) the history lengths; stats (optional) are the
 * render's; *temporal_ms / *denoise_ms (optional) as rvcp_temporal_wait / rvcp_denoise_wait
 * (denoise_ms is 0 without the flag).  tparams / dparams = NULL: the defaults.
 * Restrictions of rvcp_render_gbuffer_async. */
int rvcp_render_temporal(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                         uint32_t width, uint32_t height, const rvcp_temporal_params_t *tparams,
                         uint32_t flags, const rvcp_denoise_params_t *dparams,
                         uint8_t *out_rgba8, float *out_linear_rgb, uint32_t *out_history_len,
                         rvcp_stats_t *stats, float *temporal_ms, float *denoise_ms);

/* Drop the history rvcp_render_temporal keeps on the context. */
int rvcp_temporal_reset(rvcp_ctx_t *ctx);

/* ---------------------------------------------------------------------------------------
 * SVGF: per-pixel variance from accumulated luminance moments and a variance-guided a-trous
 * filter (opt-in; no other entry point changes).  No counterpart in the
 * reference.
 * ------------------------------------------------------------------------------------- */

/* The default parameters (chosen by tools/svgf_sweep.py).  Needs no device.
 * No counterpart in the reference. */
int rvcp_svgf_params_default(rvcp_svgf_params_t *params);

/* rvcp_temporal_accumulate_async with moments: the same step, colour and length bit for bit,
 * which also carries the first two moments of the luminance l(c) = 0.2126 r + 0.7152 g +
 * 0.0722 b through the same taps.  d_prev_moments (W*H pairs of floats) belongs to the
 * all-or-none d_prev_* set; d_out_moments (W*H pairs) receives (m1, m2): the current frame's
 * (l, l^2) where a history starts, the history's blended with max(1/n, alpha_moments_min)
 * where one continues, (0, 0) on a non-filterable pixel.  tparams / sparams = NULL: the
 * defaults; of sparams only alpha_moments_min is read, but the whole record is validated.
 * Ordered behind a render pending on the context and behind the context's previous SVGF
 * accumulation and filter.  RVCP_E_INVALID as rvcp_temporal_accumulate_async, and for SVGF
 * parameters outside their ranges, NaN, or _pad != 0.  No counterpart in the reference. */
int rvcp_svgf_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                               const void *d_cur_linear, const void *d_cur_gbuffer,
                               const void *d_prev_linear, const void *d_prev_gbuffer,
                               const void *d_prev_len, const void *d_prev_moments,
                               uint32_t width, uint32_t height,
                               const rvcp_temporal_params_t *tparams,
                               const rvcp_svgf_params_t *sparams, void *d_out_linear,
                               void *d_out_len, void *d_out_moments, void *d_rgba8_out,
                               void *stream);

/* Enqueue the variance estimate, the guided passes and the tone map on `stream`: d_linear
 * (W*H*3 floats), d_moments (W*H pairs) and d_len (W*H uint32_t) as
 * rvcp_svgf_accumulate_async leaves them, under d_gbuffer (W*H texels).  Written:
 * d_linear_out (W*H*3 floats), and when not NULL d_variance_out (W*H floats: the variance of
 * the filtered luminance after the last pass), d_feedback_out (W*H*3 floats: the colour after
 * pass 0) and d_rgba8_out (pow(clamp(c), 0.6) as RGBA8 under the context's unorm_rule).
 * Intermediates live in buffers the context owns.  params = NULL: the defaults.  Needs no
 * scene.  Ordered behind a render pending on the context and behind the context's previous
 * SVGF accumulation and filter.  RVCP_E_INVALID: NULL / zero arguments, an output that
 * overlaps an input or another output, parameters outside their ranges, NaN, _pad != 0.
 * No counterpart in the reference. */
int rvcp_svgf_filter_async(rvcp_ctx_t *ctx, const void *d_linear, const void *d_moments,
                           const void *d_len, const void *d_gbuffer, uint32_t width,
                           uint32_t height, const rvcp_svgf_params_t *params,
                           void *d_linear_out, void *d_variance_out, void *d_feedback_out,
                           void *d_rgba8_out, void *stream);

/* Wait for the context's last rvcp_svgf_accumulate_async and / or rvcp_svgf_filter_async;
 * *accumulate_ms / *filter_ms (optional) get their device times (HIP events on their streams;
 * 0 for a step that was not enqueued since the last call).  RVCP_E_INVALID when neither was.
 * No counterpart in the reference. */
int rvcp_svgf_wait(rvcp_ctx_t *ctx, float *accumulate_ms, float *filter_ms);

/* Render + G-buffer + accumulation with moments + variance + guided filter of one frame,
 * synchronously into host memory, on the context's stream and in buffers the context owns.
 * Stateful like rvcp_render_temporal, with a history of its own (colour, moments, length,
 * G-buffer, camera): the two never touch each other.  The history is dropped on the first
 * call, when width or height change, on rvcp_upload_scene / rvcp_upload_scene_file, on
 * rvcp_svgf_reset and when a call fails midway.  flags & RVCP_SVGF_FEEDBACK: the next frame's
 * colour history is pass 0's output instead of the unfiltered accumulation; moments and
 * lengths are always unfiltered.  out_rgba8 (W*H*4 bytes), out_linear_rgb (optional, W*H*3
 * floats) and out_variance (optional, W*H floats) are the filtered frame, out_history_len
 * (optional, W*H uint32_t) the history lengths; stats (optional) are the render's.
 * tparams / sparams = NULL: the defaults.  Restrictions of rvcp_render_gbuffer_async.
 * No counterpart in the reference. */
int rvcp_render_svgf(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                     uint32_t height, const rvcp_temporal_params_t *tparams,
                     const rvcp_svgf_params_t *sparams, uint32_t flags, uint8_t *out_rgba8,
                     float *out_linear_rgb, float *out_variance, uint32_t *out_history_len,
                     rvcp_stats_t *stats, float *accumulate_ms, float *filter_ms);

/* Drop the history rvcp_render_svgf keeps on the context.  No counterpart in the reference. */
int rvcp_svgf_reset(rvcp_ctx_t *ctx);

/* ---------------------------------------------------------------------------------------
 * Albedo demodulation: the filters above average irradiance = colour / albedo of the primary
 * hit instead of colour, and the albedo is multiplied back inside the tone-map store (opt-in;
 * no other entry point changes).  With the G-buffer texel's
 *   m  = material & ~RVCP_GBUFFER_EMISSIVE
 *   on = face != RVCP_GBUFFER_MISS and not (material & RVCP_GBUFFER_EMISSIVE) and
 *        m < the uploaded materials' count
 *   a  = materials[m].albedo (as uploaded), usable(a_k) = a_k > 0 and a_k < +inf
 * a pixel that is `on` gets e_k = usable(a_k) ? c_k / a_k : 0 resp. o_k = usable(a_k) ?
 * e_k * a_k : 0 per channel; every other pixel passes through.  float32, IEEE division.
 * No counterpart in the reference.
 * ------------------------------------------------------------------------------------- */

/* Enqueue the demodulation of d_linear (W*H*3 floats) under d_gbuffer (W*H texels) on
 * `stream` (NULL: the context's) into d_irradiance_out (W*H*3 floats), which may be d_linear
 * itself.  A material id outside the uploaded table is not an error: the pixel passes
 * through.  Ordered behind a render pending on the context and behind the context's previous
 * SVGF accumulation and filter.  RVCP_E_INVALID: NULL / zero arguments, W*H >= 2^31, an
 * output that overlaps an input other than d_irradiance_out == d_linear exactly;
 * RVCP_E_NO_SCENE before an upload.  Restrictions of rvcp_render_gbuffer_async.
 * No counterpart in the reference. */
int rvcp_demodulate_async(rvcp_ctx_t *ctx, const void *d_linear, const void *d_gbuffer,
                          uint32_t width, uint32_t height, void *d_irradiance_out, void *stream);

/* Enqueue the remodulation of d_irradiance (W*H*3 floats) under the same d_gbuffer, fused
 * with the store: d_linear_out (W*H*3 floats: the colour) and / or d_rgba8_out (W*H*4 bytes:
 * pow(clamp(c), 0.6) as RGBA8 under the context's unorm_rule, exactly the render's store).
 * Either output may be NULL, not both; neither may overlap an input or the other.  Ordering,
 * codes and restrictions as rvcp_demodulate_async.  No counterpart in the reference. */
int rvcp_remodulate_async(rvcp_ctx_t *ctx, const void *d_irradiance, const void *d_gbuffer,
                          uint32_t width, uint32_t height, void *d_linear_out, void *d_rgba8_out,
                          void *stream);

/* Wait for the context's last rvcp_demodulate_async and / or rvcp_remodulate_async;
 * *demodulate_ms / *remodulate_ms (optional) get their device times (HIP events on their
 * streams; 0 for a step that was not enqueued since the last call).  RVCP_E_INVALID when
 * neither was.  No counterpart in the reference. */
int rvcp_albedo_wait(rvcp_ctx_t *ctx, float *demodulate_ms, float *remodulate_ms);

/* The context's demodulation switch (default 0).  While it is 1, rvcp_render_denoised,
 * rvcp_render_temporal and rvcp_render_svgf demodulate the raw frame right after the
 * G-buffer, keep their histories (colour, and the moments of the irradiance's luminance) and
 * filter in irradiance, and end with the fused remodulate + store: out_linear_rgb is the
 * remodulated colour, out_variance the variance of the irradiance's luminance.  Changing the
 * value drops both histories (as rvcp_temporal_reset and rvcp_svgf_reset); setting the value
 * it has does nothing.  RVCP_E_INVALID while a frame is pending.
 * No counterpart in the reference. */
int rvcp_set_demodulation(rvcp_ctx_t *ctx, int on);

/* *on = the context's demodulation switch.  No counterpart in the reference. */
int rvcp_get_demodulation(rvcp_ctx_t *ctx, int *on);

/* ---------------------------------------------------------------------------------------
 * Temporal anti-aliasing: the frame is rendered through a camera rotated by a sub-pixel jitter,
 * another one each frame, and a resolve step accumulates the DISPLAYED colour (per channel the
 * linear colour clamped to [0, 1], before gamma) on the unjittered pixel grid, the history
 * clamped into the 3 x 3 neighbourhood of the current frame against ghosting (opt-in; no other
 * entry point changes).  No counterpart in the reference.
 * ------------------------------------------------------------------------------------- */

/* The jitter of frame `frame_index`, in pixels: (halton(i, 2) - 1/2, halton(i, 3) - 1/2) with
 * i = frame_index % RVCP_TAA_JITTER_PERIOD + 1, computed in double and rounded once.  Needs no
 * device.  RVCP_E_INVALID: out_jitter NULL.  No counterpart in the reference. */
int rvcp_taa_jitter(uint32_t frame_index, float out_jitter[2]);

/* *out = *base with its camera's forward rotated by `jitter` pixels of a width x height frame:
 * normalize(f^ + r^ jx / k + d^ jy / k) |forward|, with f^ = forward / |forward|, r^ =
 * normalize(forward x up), d^ = normalize(forward x r^) and k exactly as
 * rvcp_temporal_view_from_push has them; computed in double, each component rounded once.
 * Position, up, fov, near / far and time are untouched, and a zero jitter returns base's bytes
 * unchanged.  The rotation shifts the image by exactly `jitter` only at the frame's centre;
 * towards the frame's edges the shift grows by up to 1 + tan^2 of the off-axis angle (about 1.13
 * at the default 40 degree field of view) -- a jitter need not be uniform, and nothing in the
 * resolve depends on it.  Needs no device.  RVCP_E_INVALID: NULL / zero arguments, a camera
 * rvcp_temporal_view_from_push rejects, a jitter that is not finite or has a component outside
 * [-1, 1].  No counterpart in the reference. */
int rvcp_taa_jitter_push(const rvcp_push_constant_t *base, uint32_t width, uint32_t height,
                         const float jitter[2], rvcp_push_constant_t *out);

/* The default parameters: alpha_min 0.1, max_history 32, clamp 1.  Needs no device.
 * No counterpart in the reference. */
int rvcp_taa_params_default(rvcp_taa_params_t *params);

/* Enqueue one resolve step on `stream` (NULL: the context's); stateless, every buffer is the
 * caller's device memory.  d_cur_linear (W*H*3 floats) is the current frame as rendered through
 * the jittered camera (filtered or not), d_cur_gbuffer (W*H texels) its G-buffer, of which only
 * position and face are read; d_prev_resolved (W*H*3 floats) and d_prev_len (W*H uint32_t) the
 * previous call's outputs -- both NULL: no history.  cur_view / prev_view are the UNJITTERED
 * cameras of the two frames (rvcp_temporal_view_from_push); both NULL: the camera is at rest and
 * pixel p continues the history of pixel p.  Two byte-equal records take that path too, so a
 * camera at rest never resamples.  Written: d_out_resolved (W*H*3 floats; within [0, 1] when the
 * history is), d_out_len (W*H uint32_t, 1 where a history starts) and, when d_rgba8_out is not
 * NULL, pow(c, 0.6) of the result as RGBA8 under the context's unorm_rule, from the same
 * kernel.  All arithmetic is single correctly rounded f32 operations in a fixed order
 * (DESIGN.md §4.13), so the result is reproducible bit for bit.  params = NULL: the defaults.
 * Needs no scene.  A render pending on the context is not an error: the step is ordered behind
 * it, and behind the context's previous resolve.
 * RVCP_E_INVALID: NULL / zero arguments, W*H >= 2^31, an output that overlaps an input or
 * another output, one of d_prev_* or of the views without the other, alpha_min outside 0..1,
 * max_history outside 1..65535, clamp not 0 or 1 (a NaN is outside every range), _pad != 0.
 * No counterpart in the reference. */
int rvcp_taa_resolve_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *cur_view,
                           const rvcp_temporal_view_t *prev_view, const void *d_cur_linear,
                           const void *d_cur_gbuffer, const void *d_prev_resolved,
                           const void *d_prev_len, uint32_t width, uint32_t height,
                           const rvcp_taa_params_t *params, void *d_out_resolved,
                           void *d_out_len, void *d_rgba8_out, void *stream);

/* Wait for the context's last rvcp_taa_resolve_async; *taa_ms (optional) gets its device time
 * (HIP events on its stream).  RVCP_E_INVALID when no step was enqueued since the last call.
 * No counterpart in the reference. */
int rvcp_taa_wait(rvcp_ctx_t *ctx, float *taa_ms);

/* The context's TAA switch (default 0).  While it is 1, rvcp_render_temporal and
 * rvcp_render_svgf render the frame, its G-buffer and all of their own steps through
 * rvcp_taa_jitter_push(push, W, H, rvcp_taa_jitter(counter)) -- their own histories then always
 * reproject, through the jittered cameras -- and finish with rvcp_taa_resolve_async (default
 * parameters) of their final linear colour (filtered as their flags say, remodulated when the
 * demodulation switch is set) under the unjittered cameras; the resolve continues pixel by pixel
 * when the 64 camera bytes of `push` equal the previous call's.  out_rgba8 and out_linear_rgb are
 * the resolved frame; the other outputs are unchanged.  Each of the two keeps a TAA state of its
 * own (resolved colour, length, unjittered camera, frame counter), dropped -- the counter
 * restarting at 0 -- wherever its own history is dropped, and on rvcp_taa_reset.  Changing the
 * value drops both chains' histories (as rvcp_set_demodulation); setting the value it has does
 * nothing.  RVCP_E_INVALID while a frame is pending.  With the switch at 0 every output is what
 * it is without this section.  rvcp_render_denoised is stateless and not affected.
 * No counterpart in the reference. */
int rvcp_set_taa(rvcp_ctx_t *ctx, int on);

/* *on = the context's TAA switch.  No counterpart in the reference. */
int rvcp_get_taa(rvcp_ctx_t *ctx, int *on);

/* Drop the TAA states rvcp_render_temporal and rvcp_render_svgf keep on the context (their own
 * histories stay); both frame counters restart at 0.  No counterpart in the reference. */
int rvcp_taa_reset(rvcp_ctx_t *ctx);

/* ---------------------------------------------------------------------------------------
 * Temporal upsampling: the frame is traced at W / s x H / s through the jittered camera and a
 * step accumulates the displayed colour and a sample weight on the W x H grid of the unjittered
 * camera, every traced pixel dropped where its jittered centre falls (opt-in; no other entry
 * point changes).  No counterpart in the reference.
 * ------------------------------------------------------------------------------------- */

/* The default parameters: max_weight 8, init_weight 0.1, clamp 1.  Needs no device.
 * No counterpart in the reference. */
int rvcp_taau_params_default(rvcp_taau_params_t *params);

/* Enqueue one upsampling step on `stream` (NULL: the context's); stateless, every buffer is the
 * caller's device memory.  The output is width x height = W x H, the traced frame w x h =
 * W / scale x H / scale.  d_cur_linear (w*h*3 floats) is the frame rendered through the jittered
 * low-res camera; jit_view that jittered camera for a w x h frame and cur_view the UNJITTERED
 * camera for W x H (rvcp_temporal_view_from_push; both required: they place the samples).
 * d_prev_resolved (W*H*3 floats) and d_prev_weight (W*H floats) are the previous call's outputs
 * -- both NULL: no history.  prev_view is the unjittered W x H camera of the previous frame;
 * NULL, or byte-equal to *cur_view: the camera is at rest and pixel p continues the history of
 * pixel p.  Otherwise the history is reprojected through d_gbuffer_hi (W*H texels rendered
 * through the UNJITTERED camera, of which only position and face are read); it is required in
 * exactly that case and ignored in the others.  Written: d_out_resolved (W*H*3 floats, within
 * [0, 1] when the history is), d_out_weight (W*H floats: init_weight where a history starts,
 * never above max_weight) and, when d_rgba8_out is not NULL, pow(c, 0.6) of the result as RGBA8
 * under the context's unorm_rule, from the same kernel.  All arithmetic is single correctly
 * rounded f32 operations in a fixed order, so the result is reproducible bit
 * for bit.  params = NULL: the defaults.  Needs no scene.  Ordering as rvcp_taa_resolve_async:
 * behind a render pending on the context and behind the context's previous upsampling step.
 * RVCP_E_INVALID: NULL / zero arguments, scale outside 2..4, a width or height that scale does
 * not divide, W*H >= 2^31, an output that overlaps an input or another output, one of d_prev_*
 * without the other, prev_view without a history, a moved camera without d_gbuffer_hi,
 * max_weight or init_weight not finite or not > 0, clamp not 0 or 1, _pad != 0.
 * No counterpart in the reference. */
int rvcp_taa_upsample_async(rvcp_ctx_t *ctx, uint32_t scale,
                            const rvcp_temporal_view_t *jit_view,
                            const rvcp_temporal_view_t *cur_view,
                            const rvcp_temporal_view_t *prev_view, const void *d_cur_linear,
                            const void *d_gbuffer_hi, const void *d_prev_resolved,
                            const void *d_prev_weight, uint32_t width, uint32_t height,
                            const rvcp_taau_params_t *params, void *d_out_resolved,
                            void *d_out_weight, void *d_rgba8_out, void *stream);

/* Wait for the context's last rvcp_taa_upsample_async; *taau_ms (optional) gets its device time
 * (HIP events on its stream).  RVCP_E_INVALID when no step was enqueued since the last call.
 * No counterpart in the reference. */
int rvcp_taau_wait(rvcp_ctx_t *ctx, float *taau_ms);

/* The context's upsampling scale: 1 (off, the default), 2, 3 or 4.  While it is above 1 it
 * replaces the TAA resolve, whatever rvcp_set_taa says: a W x H call of rvcp_render_temporal or
 * rvcp_render_svgf (RVCP_E_INVALID when the scale does not divide W and H) runs its whole chain
 * -- render, G-buffer, demodulation, accumulation, filter, remodulation -- at w x h = W / scale x
 * H / scale through rvcp_taa_jitter_push(push, w, h, rvcp_taa_jitter(counter)), traces a W x H
 * G-buffer through the unjittered `push` on the frames whose 64 camera bytes differ from the
 * previous call's, and finishes with rvcp_taa_upsample_async at its defaults.  out_rgba8 and
 * out_linear_rgb are the W x H result; EVERY OTHER optional output (history lengths, variance)
 * keeps the traced size w x h.  Each of the two keeps an upsampling state of its own (resolved
 * colour, weight, unjittered camera, frame counter), dropped wherever its TAA state would be,
 * and on rvcp_taa_reset.  Changing the value drops both chains' histories; setting the value it
 * has does nothing.  RVCP_E_INVALID: a scale outside 1..4, a frame pending.  With the scale at
 * 1 every output is what it is without this section.  No counterpart in the reference. */
int rvcp_set_taa_upsample(rvcp_ctx_t *ctx, uint32_t scale);

/* *scale = the context's upsampling scale.  No counterpart in the reference. */
int rvcp_get_taa_upsample(rvcp_ctx_t *ctx, uint32_t *scale);

/* ---------------------------------------------------------------------------------------
 * Bounce sampling of the games101 integrator (opt-in).  The reference's README
 * lists "Important Sampling" as a TODO; its shader has no counterpart.
 * ------------------------------------------------------------------------------------- */

/* RVCP_SAMPLING_UNIFORM (the default): the shader's uniform hemisphere direction, weighted
 * f cos / (max(0.1, pdf) rr); every frame is bit-identical to the oracle.
 * RVCP_SAMPLING_COSINE: the continuation direction is normalize(n + normalize(p)), p the same
 * accepted unit-ball sample (n where the sum vanishes), drawn with density cos / pi, and the
 * path weight is the constant albedo / rr.  Everything else -- the primary ray, light sampling,
 * Russian roulette, the attenuation stop, the miss and light terms, the number and order of
 * rand() calls -- is unchanged.  The frames are NOT the oracle's: less noise per sample, more
 * traversals per frame (paths live longer), and on a scene that rays can leave a slightly
 * brighter expectation, because the shader adds its miss term unattenuated. */
#define RVCP_SAMPLING_UNIFORM 0
#define RVCP_SAMPLING_COSINE 1

/* Set the context's bounce sampling; it holds from the next render on, through every entry point
 * that renders (frames, shards, batches, the denoised / temporal / SVGF chains, the sub-contexts
 * of n_gpus > 1) and across rvcp_upload_scene.  Scene-specialised kernels are compiled for the
 * new mode by the first render after a change (cached per mode, in the process and on disk).
 * Changing the value drops the histories of rvcp_render_temporal and rvcp_render_svgf; setting
 * the value it has does nothing.  RVCP_E_INVALID: a null context, an unknown value, a frame
 * pending.  RVCP_E_UNSUPPORTED: RVCP_SAMPLING_COSINE on a RVCP_INTEGRATOR_LEGACY context
 * (ray_tracer.comp's diffuse scatter is cosine-weighted already). */
int rvcp_set_sampling(rvcp_ctx_t *ctx, int32_t sampling);

/* *sampling = the context's bounce sampling. */
int rvcp_get_sampling(rvcp_ctx_t *ctx, int32_t *sampling);

/* ---------------------------------------------------------------------------------------
 * Material scattering on meshes (opt-in).  ray_tracer_games101_branch.comp
 * defines the four material types (:22-25) and reads one: the light test (:425).  Every other
 * face is shaded as a Lambertian surface, whatever rvcp_material_t::ty says.
 * ------------------------------------------------------------------------------------- */

/* RVCP_MATERIALS_LAMBERTIAN (the default): the shader's behaviour, bit-identical to the oracle.
 * RVCP_MATERIALS_SCATTER: ray_trace_games101 (:406-482) with these changes and no other.
 *   - At a hit on a Metal or Dielectric face no light sample is drawn and no shadow ray traced.
 *     The roulette comes first (:462), then the new direction and colour (nd, na) are
 *     material_scatter's for the type (ray_tracer.comp:515-581: metal reflects, flips the
 *     reflection into the normal's hemisphere and redraws normalize(r + fuzz * unit vector) while
 *     it points below the surface, na = albedo; dielectric picks its ratio by the hit's `outward`
 *     flag, tests total internal reflection, compares one rand() with Schlick only when
 *     refraction is possible, na = 1), attenuation *= na / RR_PROBABILITY, and the next ray is
 *     Ray(p + nd * EPS, nd, RAY_T_MIN, RAY_T_MAX).  The metal redraw is bounded: after 16
 *     rejected draws nd = normalize(r).
 *   - The emission rule (:426) becomes depth == 0 || the previous vertex was specular: a light
 *     seen in a mirror or through glass counts once.  The miss term (:424) is unchanged.
 *   - Shadow rays are unchanged: a metal or glass face blocks them like any face.
 * While it is set, rvcp_trace_paths(_async) run its kernel, and rvcp_render, rvcp_render_async
 * and rvcp_render_shard_async (shard_count = 1) render through it: the frame's primary rays and
 * seeds, that kernel, the tone map -- the generic scan or the BVH, not the scene-specialised
 * kernels.  rvcp_stats_t::kernel_variant is then 11, and traversals is counted by the kernel.
 * rvcp_render_denoised, rvcp_render_temporal and rvcp_render_svgf run on top unchanged (their
 * G-buffer is still the primary hit).  RVCP_E_UNSUPPORTED, before any launch: n_frames > 1,
 * shard_count > 1, rvcp_render_spp_map_async (and so the adaptive switch).  Ray queries and the
 * G-buffer do not depend on the mode.
 * A scene is accepted only if every Metal material has a finite fuzz in [0, 1] and every
 * Dielectric a finite refraction_ratio > 0: rvcp_upload_scene while the mode is set, and
 * rvcp_set_materials on a loaded scene, return RVCP_E_INVALID naming the material otherwise. */
#define RVCP_MATERIALS_LAMBERTIAN 0
#define RVCP_MATERIALS_SCATTER 1

/* Set the context's materials mode; it holds from the next render or path query on and across
 * rvcp_upload_scene.  Changing the value drops the temporal, SVGF, TAA and upsampling
 * histories; setting the value it has does nothing.  RVCP_E_INVALID: a null context, an unknown
 * value, a frame pending, a loaded scene with an invalid fuzz or refraction_ratio.
 * RVCP_E_UNSUPPORTED for RVCP_MATERIALS_SCATTER on a RVCP_INTEGRATOR_LEGACY context (mode 2
 * scatters by material already), an n_gpus > 1 context, or one whose sampling is
 * RVCP_SAMPLING_COSINE; rvcp_set_sampling(RVCP_SAMPLING_COSINE) is refused likewise while the
 * mode is set.  No counterpart in the reference. */
int rvcp_set_materials(rvcp_ctx_t *ctx, int32_t materials);

/* *materials = the context's materials mode. */
int rvcp_get_materials(rvcp_ctx_t *ctx, int32_t *materials);

/* ---------------------------------------------------------------------------------------
 * Adaptive sampling (opt-in): frames traced with a per-pixel sample count, a
 * plan step that makes the counts from a filtered frame's variance, and a switch that closes
 * the loop inside rvcp_render_svgf.
 * ------------------------------------------------------------------------------------- */

/* rvcp_render_async with a per-pixel sample count: d_spp_map holds width x height uint32_t in
 * device memory, row-major, and pixel p is traced with s_p = min(max(map[p], 1),
 * RVCP_SPP_MAP_MAX) samples of its own RNG stream -- bit for bit the pixel of a frame rendered
 * with cfg.spp = s_p (and of the oracle's, with RVCP_SAMPLING_UNIFORM); a uniform map of s is
 * rvcp_render_async at cfg.spp = s.  cfg.spp is not read; spp_hint (1..RVCP_SPP_MAP_MAX) stands
 * in for it where the schedule and the grid are chosen and changes no bit of the frame.  The
 * map is read by the frame's first kernel: it must stay unchanged until rvcp_wait.  The frame
 * is the context's pending frame (rvcp_wait / rvcp_sync_stats: samples = sum of s_p, traversals
 * = traversals_executed + sum of (s_p - 1)) and is ordered like rvcp_render_async's; the
 * context's bounce sampling holds (rvcp_set_sampling).  Scene-specialised kernels are compiled
 * for map renders by the first one (cached per bounce sampling, in the process and on disk).
 * RVCP_E_INVALID: a null or zero argument, a hint outside 1..RVCP_SPP_MAP_MAX, W*H >= 2^31, a
 * frame pending.  RVCP_E_NO_SCENE before an upload.  RVCP_E_UNSUPPORTED: a
 * RVCP_INTEGRATOR_LEGACY context, n_gpus > 1, a resolved schedule of 1 or 2 (the map is read by
 * the pre-pass: schedules 3-6, 10 and the BVH path kernel). */
int rvcp_render_spp_map_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                              uint32_t width, uint32_t height,
                              const void *d_spp_map /* W*H uint32_t */, uint32_t spp_hint,
                              void *d_rgba8, void *d_linear_rgb, void *stream);

/* The defaults: the best row on average of tools/adaptive_sweep.py. */
int rvcp_adaptive_params_default(rvcp_adaptive_params_t *params);

/* The plan step (stateless, on the caller's buffers): the map of the next frame from a frame's
 * variance d_variance (W*H float), the colour it belongs to d_linear (W*H*3 float, in the same
 * domain), its history lengths d_len (W*H uint32_t, or NULL: 1 everywhere) and its G-buffer.
 * Per pixel q = floor(2^20 min(w, weight_cap) / weight_cap) with w = v / (lum(c)^2 + epsilon) /
 * n, every operation a float32 operation rounded once, and q = 0 for a pixel that is not
 * filterable (a miss, emissive), reads a non-finite float, has v not > 0 or n = 0.  With S the
 * integer sum of q, B = floor(mean_spp W H) and E = B - spp_min W H: s = spp_min + min(E q / S,
 * spp_max - spp_min) in unsigned 64-bit integers, and with S = 0 every pixel gets
 * min(spp_min + E / (W H), spp_max).  So spp_min <= s <= spp_max and sum(s) <= B always; what the
 * spp_max clamp cuts off is not handed to other pixels.  params NULL: the defaults.  Ordered
 * behind a render pending on this context and behind the context's previous plan step; the
 * output may overlap no input.  RVCP_E_INVALID: a null or zero argument, W*H >= 2^31, parameters
 * out of range (NaN included), _pad != 0, an overlap. */
int rvcp_spp_plan_async(rvcp_ctx_t *ctx, const void *d_variance /* W*H float */,
                        const void *d_linear /* W*H*3 float */, const void *d_len /* W*H u32, or NULL: 1 */,
                        const void *d_gbuffer, uint32_t width, uint32_t height,
                        const rvcp_adaptive_params_t *params, void *d_spp_map_out, void *stream);

/* Wait for the plan step: its time and the sum of the map it wrote (either may be NULL). */
int rvcp_spp_plan_wait(rvcp_ctx_t *ctx, float *plan_ms, uint64_t *planned_samples);

/* The switch (off by default; params NULL: off).  While it is on, rvcp_render_svgf -- and only
 * it -- traces its raw frame with rvcp_render_spp_map_async through a map the context keeps, and
 * after the filter plans the next frame's map with rvcp_spp_plan_async from the frame's own
 * filtered colour (irradiance when demodulating), variance, history lengths and G-buffer, at the
 * traced size; `stats` are the map render's.  The map is in the previous frame's pixel grid and
 * is not reprojected.  Wherever the SVGF history is dropped (the first call, a size change, an
 * upload, rvcp_svgf_reset, a failed call, the switches that drop it) the map is dropped with it
 * and the frame is traced through the uniform map of min(max(floor(mean_spp), spp_min),
 * spp_max).  Turning the switch on or off or changing the parameters drops the map, not the SVGF
 * history.  RVCP_E_UNSUPPORTED: a RVCP_INTEGRATOR_LEGACY or n_gpus > 1 context.  RVCP_E_INVALID:
 * parameters out of range (NaN included), _pad != 0, a frame pending. */
int rvcp_set_adaptive(rvcp_ctx_t *ctx, const rvcp_adaptive_params_t *params /* NULL: off */);

/* *on = the switch, *out_params = its parameters (the defaults while it is off); either may be
 * NULL. */
int rvcp_get_adaptive(rvcp_ctx_t *ctx, int *on, rvcp_adaptive_params_t *out_params);

/* The map the last frame of rvcp_render_svgf was traced with under the switch: out_map (host,
 * *out_width x *out_height uint32_t; may be NULL to ask for the size alone).  RVCP_E_INVALID
 * before any such frame. */
int rvcp_adaptive_last_map(rvcp_ctx_t *ctx, uint32_t *out_map, uint32_t *out_width, uint32_t *out_height);

#ifdef __cplusplus
}
#endif

#endif /* RVCP_H */
