// rvcp_internal.h -- device-side data layout shared by the host runtime (rvcp_host.cpp) and
// the gfx950 kernels (rvcp_kernels.hip).  Not part of the C-ABI.
#pragma once

#ifndef __HIPCC_RTC__             // hipRTC (rvcp_jit.cpp) provides the fixed-width types
#include <stdint.h>

#include <vector>
#else
using __hip_internal::int32_t;
using __hip_internal::uint8_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#endif

// functions the host and the kernels share: qualified under hipcc / hipRTC, plain elsewhere
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define RVCP_HOST_DEVICE __host__ __device__
#else
#define RVCP_HOST_DEVICE
#endif

namespace rvcp {

// Wave width on CDNA4.
constexpr int kWave = 64;
// Threads per workgroup of the path-tracing kernel (4 independent waves).
constexpr int kBlock = 256;
// schedule 10 (LDS-tiled scan with the workgroup ray pool): waves per workgroup
#ifndef RVCP_TILED_POOL_WAVES
#define RVCP_TILED_POOL_WAVES 8
#endif
constexpr int kTiledPoolWaves = RVCP_TILED_POOL_WAVES;
// LDS state columns of the path kernels (path_body LDS_STATE): a_p 0-2, nee_C 3-5, nee_dist 6,
// acc 7-9, att 10-12, col 13-15
constexpr int kStateCols = 16;
// Pixels a wave takes from the frame queue per atomic.
constexpr uint32_t kChunk = 64;
// Small frames: the grid is sized so that a wave starts with at least kMinStatic pixels, and
// the pixels are spread over all those waves (more waves per SIMD to hide latency).
constexpr uint32_t kMinStatic = 8;
// Static chunks: full 64-pixel waves (fewest wave-instructions for the work) unless that
// leaves fewer than two waves per SIMD, in which case the pixels are spread over up to two
// waves per SIMD, at least kMinStatic each (latency hiding matters more for tiny frames).
// Returns the waves that get a static chunk and its size.  One definition for the host's frame
// plan (rvcp_frame_plan.cpp, also built without HIP) and the kernels.
RVCP_HOST_DEVICE inline void static_split(uint32_t n, uint32_t grid_waves, uint32_t n_simds,
                                          uint32_t &waves, uint32_t &chunk) {
    uint32_t w = (n + kChunk - 1) / kChunk;
    const uint32_t spread = (n + kMinStatic - 1) / kMinStatic;
    const uint32_t floor_w = spread < 2u * n_simds ? spread : 2u * n_simds;
    if (w < floor_w) w = floor_w;
    if (w > grid_waves) w = grid_waves;
    if (w < 1u) w = 1u;
    uint32_t c = (n + w - 1) / w;
    chunk = c < 1u ? 1u : (c > kChunk ? kChunk : c);
    waves = w;
}
// Frame-queue grabs after a wave's static chunk: what the wave consumes in kChunkWindow
// s_memrealtime ticks (100 MHz), between kMinChunk and kDynChunk pixels (queue_take,
// DESIGN.md §4.1).
constexpr uint32_t kDynChunk = 64;
constexpr uint32_t kMinChunk = 2;
constexpr uint32_t kChunkWindow = 10000;    // 100 us
// Kernel schedules (rvcp_config_t::kernel_variant): 1 = one ray per lane per iteration,
// 2 = shadow + continuation ray per lane per iteration, 3 = primary pre-pass kernel + the
// variant-2 loop over surface pixels only.
// 4 = variant 3 with the triangle scan staged through LDS tiles shared by the workgroup
// (the automatic choice for meshes of kTiledMinFaces faces or more on frames of
// kTiledDualMinSamples pixel-samples or more).
// 5 = variant 4 with one ray per lane per iteration (the shadow ray, then the path ray), so no
// ray slot is empty; the automatic choice for large meshes on smaller frames, whose rays do not
// fill the chip twice over.
// 6 = variant 3 compiled for 6 waves per SIMD instead of 5 (80 VGPRs, a few spills): faster
// once the frame is large enough that latency hiding beats the spills (automatic from
// kWideMinSamples pixel-samples per frame).
// 10 = variant 4 with the workgroup ray pool: the rays of a workgroup of kTiledPoolWaves waves
// are scanned against each LDS tile in 64-ray passes shared out over its waves (the automatic
// choice wherever 4 was).  (7 and 8 are the stats codes of the BVH and mode-2 kernels, 9 is
// unused: a non-tiled pool measured slower)
constexpr int kDefaultVariant = 3;
constexpr int kMaxVariant = 10;
// d_counters (u64 words): executed traversals, queue head, wave iterations, surface-list
// length, and at kClockWord (a cache line of its own) the path kernel's clock stamps
// (shader-clock ticks, 100-MHz ticks; clock_stamp in rvcp_kernels.hip)
constexpr int kCounterWords = 32;
constexpr int kClockWord = 16;
// ... and, from the pre-pass of a map render (RVCP_SPP_MAP), the sum of the
// frame's clamped per-pixel sample counts
constexpr int kSppSumWord = 4;
constexpr int kTiledPoolVariant = 10;
constexpr int variant_block(int v) { return v == kTiledPoolVariant ? kTiledPoolWaves * kWave : kBlock; }
constexpr uint64_t kWideMinSamples = 8ull << 20;   // auto: variant 6 from 8 Msamples per frame
// auto, scene-specialised scan: its 6-wave build (variant 6) from 256 Msamples per frame -- C4's
// 2048^2 SPP=64 frame 23.39 -> 23.00 ms, while C3 (31 M) is 0.3 % and C2 6 % slower at 6 waves
// (profiles/history/r04z_ab_waves6.log)
// A batch's pre-passes run as one launch (one frame per grid row) for frames up to this many
// pixels, whose per-frame pre-pass is too small to fill the GPU (C2: 0.1666 -> 0.1645 ms per
// frame); larger frames keep one launch per frame (C3 at 60 frames: 2.810 vs 2.827 ms,
// profiles/history/r04pb_ab_prebatch.log).
constexpr uint32_t kPrepassBatchMaxPixels = 512u * 1024u;
constexpr uint64_t kSpecWideMinSamples = 256ull << 20;
constexpr int kOccupancyBvh = 100;          // KernelBuild::occupancy code of the BVH kernel
#ifndef RVCP_TILE
#define RVCP_TILE 256
#endif
constexpr uint32_t kTile = RVCP_TILE;       // triangles per LDS tile (12 KiB at 256)
constexpr uint64_t kTiledDualMinSamples = 1ull << 19;   // auto: variant 4 rather than 5 from here
                                            // (4 wins at 512x512x4, 5 at 256x256x4)
constexpr uint32_t kTiledWideMinFaces = 64;   // auto: variant 4 above this many faces on
                                            // frames of kTiledDualMinSamples or more (F = 72:
                                            // 4 beats 3 and 6 from 2 Msamples)
constexpr uint32_t kTiledMinFaces = 256;   // auto: variant 5 from here (measured crossover
                                            // vs variant 3 at ~230 faces)

// One triangle as the brute-force scan reads it: v0, e1 = v1 - v0, e2 = v2 - v0, computed on
// the host with the same float subtractions the shader performs per test
// (ray_tracer_games101_branch.comp:247-248), so the scan is bit-identical while reading
// 36 algorithmic bytes per test.  Padded to 48 B (three 16-B rows).
struct alignas(16) TriRecord {
    float v0[3];
    float e1[3];
    float e2[3];
    float pad[3];
};
static_assert(sizeof(TriRecord) == 48, "TriRecord is 48 B");

// Scenes up to this many faces get the scene-specialised scan (rvcp_jit.cpp; the unrolled code
// grows with the face count, and the specialised kernels keep the scene in LDS arrays of this
// size).
constexpr uint32_t kJitMaxFaces = 64;

// One entry of the light table: a luminous face as sample_light_games101 sees it
// (ray_tracer_games101_branch.comp:384-404), with the std140 id quirk already applied.
struct alignas(16) LightRecord {
    float cum;          // running emit_area_sum after this entry (second loop, :396-399)
    uint32_t face;      // face index
    float pad0[2];
    float v0[4];        // positions of the face's three vertices (sample_in_face :315-317)
    float v1[4];
    float v2[4];
    float n[4];         // normalize(vertices[face.x].normal)  (:325)
    float le[4];        // materials[face.material_id].albedo  (:437)
};
static_assert(sizeof(LightRecord) == 96, "LightRecord is 96 B");

// A pixel whose primary ray hit a non-emissive surface, as the primary pre-pass hands it to
// the path kernel (variant 3): the cached primary hit record (:421-431 at depth 0) and the
// pixel's RNG seed.
struct alignas(16) SurfRecord {
    float pos[3];
    uint32_t pix;
    float nrm[3];
    float seed;         // srand's seed of the pixel (:153-155), computed once by the pre-pass
    float alb_pi[3];    // albedo / pi of the hit material
    uint32_t mat;
};
static_assert(sizeof(SurfRecord) == 48, "SurfRecord is 48 B");

// Per-face shading data, gathered by index once per traversal for the nearest face only:
// the three vertex normals (interpolated at :262-266), the face material (:272) with its type
// and albedo / PI.  One independent 64-B gather instead of face -> vertices -> material.
struct alignas(16) FaceShade {
    float n0[3];
    uint32_t mat;
    float n1[3];
    uint32_t ty;
    float n2[3];
    uint32_t pad0;
    float alb_pi[3];
    uint32_t pad1;
};
static_assert(sizeof(FaceShade) == 64, "FaceShade is 64 B");

// Per-material record: albedo + type (MaterialBuffer, :74-83) and albedo / PI, the value
// lambertian_brdf_eval returns (:346), divided once on the host with the same float division.
struct alignas(16) MatRecord {
    float albedo[3];
    uint32_t ty;
    float alb_pi[3];
    uint32_t pad;
};
static_assert(sizeof(MatRecord) == 32, "MatRecord is 32 B");

// Opt-in BVH (rvcp_config_t.accel = RVCP_ACCEL_BVH).  The builder makes a binary tree whose
// nodes hold both children's boxes; child reference: >= 0 an internal node, < 0 a leaf
// ~ref = first << 5 | (count - 1) over the leaf-ordered triangle array.  Boxes are enlarged at
// build time (bvh_build) so that a triangle the exact test accepts is never culled by rounding
// in the box test.  The device traverses the 4-wide tree bvh4_collapse makes of it.
struct alignas(16) BvhNode {
    float lbox[6];      // left child: lo xyz, hi xyz
    float rbox[6];      // right child
    int32_t left, right;
    int32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode is 64 B");
// at most this many triangles per BVH leaf: 2 since round 5 -- with the node-phase break
// (rvcp_kernels.hip) the 4-triangle leaves' tests cost more than the extra node steps of 2
// (C5 BVH 52.0 -> 47.0 ms; 1: 46.5 ms for 1.8x the nodes; profiles/history/r05zc_ab_bvhleaf.log,
// r05zd_ab_bvhleaf2.log)
#ifndef RVCP_BVH_LEAF_MAX
#define RVCP_BVH_LEAF_MAX 2
#endif
constexpr int kBvhLeafMax = RVCP_BVH_LEAF_MAX;
constexpr uint32_t kBvhPadId = 0xFFFFFFFFu;   // padding slot of the leaf order (even leaf starts)
constexpr int kBvhStack = 32;           // traversal stack entries per lane
// Relative slack of the slab comparison in the traversal of primary rays
// (bvh_nearest<.., PRIMARY>): a child box is entered iff tn <= tf + kBvhSlabSlack * |tf| (tf
// already clamped to the nearest hit so far).  Shadow and path rays start on a surface, inside
// the scene, and need none.  The slab times carry the rounding of their decode, (origin - o) *
// inv and scale * inv with a 1-ulp reciprocal, and the nearest hit's t its own few ulp; relative
// to t that is a few 2^-24, which from an origin some hundred scene diagonals away exceeds the
// build's box enlargement (1e-5 of the diagonal) -- the traversal then lost hits the scan
// keeps.  Measured on the CPU model
// (tools/bvh4_check.cpp, tests/test_bvh_adversarial_cpu.py: 24 108 rays from up to 1000 diagonals
// over 41 adversarial meshes): a slack of 2^-23 is the smallest power of two that loses none of
// them (2^-24 still loses some); the device's v_rcp_f32 adds up to 2^-23 to the model's IEEE
// reciprocal, and 2^-21 is twice that sum.  Only ever conservative: it enters more boxes.
constexpr float kBvhSlabSlack = 0x1p-21f;
// The ray queries' traversal stack (ray_query_kernel): the private array, or (true) LDS columns.
// Both are built; the measurement that chose is in DESIGN.md §4.19.
constexpr bool kRayQueryLdsStack = true;

// The traversed tree: up to 4 children per node, boxes stored per axis so one node is seven
// 16-byte loads; a step tests the four boxes, pushes the hit children but the nearest (farthest
// first) and descends into the nearest.  Unused child slots hold an unreachable box (a point
// at 3e38) and the leaf reference ~0 (triangle 0 again: a repeated test never changes the hit).
// ~0 is also a real leaf (slot 0, one triangle), so it is pad[child] that says which slots are
// used.
struct alignas(16) Bvh4Node {
    float lo[3][4];     // lo[axis][child]
    float hi[3][4];
    int32_t ref[4];
    int32_t pad[4];     // 1: the child slot is used, 0: unused
};
static_assert(sizeof(Bvh4Node) == 128, "Bvh4Node is 128 B");

// The same node with its child boxes quantised to bytes (bvh4_quantize): per axis the children's
// bounds are origin + q * scale with scale a power of two, lo rounded down and hi up (so every
// box contains its Bvh4Node box); byte c of qlo[axis] / qhi[axis] is child c.  Unused children
// are inverted on every axis (qlo = 255 > qhi = 0, which no used child has: its qhi >= qlo) and
// keep the reference ~0, so that whatever enters one only tests the triangle at slot 0 again,
// inside the leaf buffer.  The inversion alone does not keep a ray out: it is 255 * scale * inv
// in slab time, which the rounding of (origin - o) * inv swallows once the ray's origin is 2^24
// node extents away on every axis (fma(255, a, b) == b), and an entered unused slot is a push
// that bvh4_collapse's stack bound did not count.  The traversal of primary rays therefore
// keys a slot with qlo > qhi +inf (bvh_nearest<.., PRIMARY>, rvcp_kernels.hip); what is left
// for the other rays is described there.  64 B: four 16-B loads per traversal step instead of
// seven.
struct alignas(16) Bvh4QNode {
    float origin[3];
    float scale[3];
    uint32_t qlo[3];
    uint32_t qhi[3];
    int32_t ref[4];
};
static_assert(sizeof(Bvh4QNode) == 64, "Bvh4QNode is 64 B");

// Frame-constant parameters of one render launch.
struct FrameArgs {
    // camera, precomputed on the host exactly as sample_ray (:217-235) computes it
    float cam_pos[3];
    float u[3];          // normalize(cross(fwd, up)) * w
    float v[3];          // normalize(cross(fwd, u)) * h
    float pos[3];        // cam_pos + fwd * t_near
    float base_len;      // length(pos - cam_pos)
    float t_near, t_far;
    float time;          // push-constant time (RNG seed input)
    uint32_t width, height;
    uint32_t shard_index, shard_count;
    uint32_t n_pixels;   // pixels owned by this shard (rows * width)
    uint32_t spp, max_bounces;
    float att_stop, t_min, t_max, rr, eps;
    uint32_t n_faces, n_lights;
    float light_total, light_pdf;
    // the BRDF update's divisor max(0.1, pdf) * rr (:465-471) for pdf = 1/(2 pi) (cos > 0) and
    // pdf = 0, and their IEEE reciprocals: frame constants, so the update divides by a known
    // reciprocal (divs_y) instead of computing rcp_ieee per event
    float brdf_den[2], brdf_rcp[2];
    // every light record samples the same face (the std140 id quirk on the Cornell box maps
    // both entries to face 0): nee_sample's pick cannot change the sample, so it reads record 0
    uint32_t lights_same;
    // every triangle's scan denominator is +-0 or within [2^-126, 2^126] for rays passing
    // dir_fast_ok (scan_rcp_fast_scene): the generic scans may take 1/den without the class check
    uint32_t rcp_fast;
    // the scene has a metal material (type 1): mode 2's scatter needs the reflected direction
    uint32_t has_metal;
    uint32_t static_chunks;  // pixels handed out statically (one chunk per wave)
    uint32_t static_chunk;   // pixels of each wave's static chunk (<= kChunk)
    uint32_t n_simds;        // SIMDs of the device (CUs x 4), for static_split
    uint32_t want_linear;
    int32_t variant;         // kernel schedule (rvcp_config_t::kernel_variant, resolved)
    uint32_t n_spheres;      // integrator RVCP_INTEGRATOR_LEGACY only
    uint32_t n_mats;
    uint32_t dyn_chunk;      // largest frame-queue grab after the static chunk
    uint32_t chunk_min;      // smallest grab
    uint32_t chunk_window;   // grab = pixels this wave consumes in chunk_window ticks (10 ns)
    int32_t accel;           // RVCP_ACCEL_*
    int32_t bvh_root;        // root reference (see BvhNode) when accel == RVCP_ACCEL_BVH
    uint32_t bvh_n4;         // Bvh4Node offset of the quantised nodes in the node buffer (0)
    uint32_t bvh_slots;      // TriRecord offset of the packed 10-float leaf records (0: buffer start)
    // faces [0, bvh_prefix) are not in the BVH: every ray tests them first, with the
    // scene-specialised scan where the module has one, else the generic test (the hybrid of
    // DESIGN.md §4.6); 0 = the BVH holds every face
    uint32_t bvh_prefix;
    // small frames (path kernels of schedules 3/6): when the surface list fits the resident
    // lanes, spread it over every resident wave, at least spread_min pixels each (0 = off),
    // and let waves with <= 32 rays split each ray's scan over R lanes from the first
    // iteration (early_tail), not only once the queue is empty
    uint32_t spread_min;
    uint32_t early_tail;
    // index of this frame's first pixel in the outputs (rvcp_render_frames_async: frame k of a
    // batch starts at k x the largest shard's pixels; 0 for a single frame)
    uint32_t pix_base;
    // integrator mode 2 batches (one kernel over n frames; rvcp_render_frames_async): queue
    // pixel p is pixel p % frame_pixels of frame p / frame_pixels, whose camera and time are
    // the 16 floats at batch_cams + 16 * frame (FrameCam order: cam_pos, u, v, pos, base_len,
    // t_near, t_far, time) and whose outputs start frame_stride pixels after the previous
    // frame's; batch_cams == nullptr for a single frame
    uint32_t frame_pixels, frame_stride;
    // cosine-weighted bounce sampling (RVCP_SAMPLING_COSINE): the attenuation
    // update's factor PI_F / rr, one IEEE division on the host; read by the cosine builds of the
    // kernels only.  It fills the padding in front of the pointer: no other member moves.
    float cos_k;
    const float *batch_cams;
    // debug build of the library only: per-wave {start, queue exhausted, end, iterations,
    // shader-clock start, shader-clock end}
    // of the path kernel, s_memrealtime ticks (100 MHz); nullptr otherwise
    unsigned long long *timeline;
};
static_assert(sizeof(FrameArgs) == 256, "FrameArgs is 256 B (cos_k sits in former padding)");

#ifndef __HIPCC_RTC__
// rvcp_bvh.cpp: build the BVH over n faces (three vertex positions each); returns the depth.
// pad_abs, if given, receives the absolute part of the build's box enlargement (the checker's
// classifier, tools/bvh4_check.cpp, judges a lost hit against the pad the build really used).
int bvh_build(const float (*pos)[3][3], uint32_t n, std::vector<BvhNode> &nodes,
              std::vector<uint32_t> &order, int32_t &root, float *pad_abs = nullptr);
// Collapse the binary tree into the 4-wide one, keeping the traversal stack within
// kBvhStack entries; returns that stack bound.
int bvh4_collapse(const std::vector<BvhNode> &nodes, int32_t root, std::vector<Bvh4Node> &out,
                  int32_t &root4);
// rvcp_bvh.cpp: the byte-quantised copy of a collapsed tree (same indices and refs).
void bvh4_quantize(const std::vector<Bvh4Node> &in, std::vector<Bvh4QNode> &out);
// rvcp_bvh.cpp: how many leading faces are "big" (box extent above the split-clipping
// threshold: max(8 x the median extent, scene diagonal / 16)), at most `cap`; the hybrid tests
// them with the specialised scan and builds the BVH over the rest.
uint32_t bvh_big_prefix(const float (*pos)[3][3], uint32_t n, uint32_t cap);

#endif  // __HIPCC_RTC__
}  // namespace rvcp

#ifndef __HIPCC_RTC__
namespace rvcp {
// One launch of the games101 kernels.  The pre-pass family (schedules 3-6, 10, the BVH path
// kernel) reads all of it: args[0 .. n_frames) is one FrameArgs per frame of the batch (pix_base =
// k x frame_stride); one pre-pass per frame into one surface list, main_event recorded, one path
// kernel, one tone map over n_frames x frame_stride pixels (n_pixels when n_frames == 1).
// Schedules 1 and 2 read args[0], the scene, the outputs, counters, grid_blocks and stream.
struct PathLaunch {
    const FrameArgs *args;
    uint32_t n_frames, frame_stride;
    const TriRecord *tri;
    const void *faces, *verts;
    const MatRecord *mats;
    const LightRecord *lights;
    const float *gamma_t;
    uint32_t *out_rgba;
    float *out_lin;
    unsigned long long *counters;
    SurfRecord *surf;
    const FaceShade *shade;
    const Bvh4Node *bvh_nodes;
    const TriRecord *bvh_tris;
    uint32_t grid_blocks;
    void *stream, *main_event;
    // the scene-specialised path kernel and pre-pass (rvcp_jit.cpp), or null for the built-in
    // ones; their module must have been compiled for this build (JitSpec's sampling and spp_map)
    void *spec_path_fn, *spec_pre_fn;
    const float *cams;          // a batch's cameras in device memory: one pre-pass launch, or null
    // a map build (RVCP_SPP_MAP = 1): the frame's per-pixel sample counts,
    // n_pixels words of device memory, clamped by the pre-pass; null otherwise
    const uint32_t *spp_map;
};
// One static build of the games101 kernels: rvcp_kernels.hip compiled per bounce sampling
// (RVCP_SAMPLING) and with or without the per-pixel sample count (RVCP_SPP_MAP).
struct KernelBuild {
    int (*launch)(const PathLaunch &);           // schedules 1 and 2; null in a map build
    int (*launch_prepass)(const PathLaunch &);   // the pre-pass family
    // resident workgroups per CU of a schedule's kernel, or of the BVH path kernel
    // (kOccupancyBvh); a map build knows schedules 3, 4, 5, 6, 10 and kOccupancyBvh
    int (*occupancy)(int variant, int *blocks_per_cu);
};
// kKernelBuilds[sampling][map] (rvcp_host.cpp), over the one object each of rvcp_kernels.hip,
// rvcp_kernels_map.hip, rvcp_kernels_cosine.hip and rvcp_kernels_cosine_map.hip exports
extern const KernelBuild *const kKernelBuilds[2][2];
}  // namespace rvcp

// The launchers every build shares (defined in rvcp_kernels.hip and the post-process files),
// called by rvcp_host.cpp.
extern "C" {
extern const rvcp::KernelBuild rvcp_games101_build, rvcp_games101_map_build,
    rvcp_games101_cosine_build, rvcp_games101_cosine_map_build;
// Integrator RVCP_INTEGRATOR_LEGACY (ray_tracer.comp): materials / spheres are the raw
// rvcp_material_t / rvcp_sphere_t arrays, unorm_t the UNORM8 threshold table.
int rvcp_launch_legacy(const rvcp::FrameArgs *args, const rvcp::TriRecord *tri,
                       const rvcp::FaceShade *shade, const void *spheres, const void *materials,
                       const float *unorm_t, uint32_t *out_rgba, float *out_lin,
                       unsigned long long *counters, uint32_t grid_blocks, void *stream,
                       void *spec_legacy_fn);
int rvcp_legacy_occupancy(int *blocks_per_cu);
// mandelbrot.comp (rvcp_mandelbrot.hip)
int rvcp_launch_mandelbrot(float pos_x, float pos_y, float scale, uint32_t width,
                           uint32_t height, const float *unorm_t, uint32_t *out_rgba,
                           float *out_value, void *stream);
// The G-buffer of one frame (rvcp_render_gbuffer_async): args->n_pixels texels of 32 B into out
int rvcp_launch_gbuffer(const rvcp::FrameArgs *args, const rvcp::TriRecord *tri,
                        const rvcp::FaceShade *shade, const rvcp::Bvh4Node *bvh_nodes,
                        const rvcp::TriRecord *bvh_tris, void *out, void *stream);
// Ray queries (rvcp_trace_rays_async): args->n_pixels rays of 32 B from `rays`,
// traced over args' faces (n_faces, or bvh_prefix and the tree with args->accel); `any` = 0: one
// 16-B rvcp_ray_hit_t per ray into out, 1: one uint32_t.  lds_stack: the tree's stack in LDS
// columns instead of the private array (the A/B of §4.19; the product passes kRayQueryLdsStack).
int rvcp_launch_ray_query(const rvcp::FrameArgs *args, const rvcp::TriRecord *tri,
                          const rvcp::Bvh4Node *bvh_nodes, const rvcp::TriRecord *bvh_tris,
                          const void *rays, int any, int lds_stack, void *out, void *stream);
// The primary rays of pixels [first, first + count) of args' frame as rvcp_ray_t records into out
// (rvcp_primary_rays_async, rvcp_pick)
int rvcp_launch_primary_rays(const rvcp::FrameArgs *args, uint32_t first, uint32_t count, void *out,
                             void *stream);
// Path queries (rvcp_trace_paths_async): the radiance along args->n_pixels rays
// of 32 B from `rays` with one float seed each, args->spp samples per ray with args' shading
// parameters, three floats per ray into out.  A persistent grid over a queue, as the render
// kernels': the launcher sizes it (at most the resident workgroups, or grid_waves_per_simd > 0
// waves per SIMD) and fills args' queue members itself; static_lanes (the debug build's A/B of
// §4.20, 0 in the product): one ray per lane in a grid of as many lanes as rays instead.
// counters: four u64 words of the query's own, zeroed on the stream before the launch
// ([0] traversals, [1] queue head, [2] iterations).
int rvcp_launch_path_query(const rvcp::FrameArgs *args, const rvcp::TriRecord *tri,
                           const rvcp::FaceShade *shade, const rvcp::MatRecord *mats,
                           const rvcp::LightRecord *lights, const rvcp::Bvh4Node *bvh_nodes,
                           const rvcp::TriRecord *bvh_tris, const void *rays, const void *seeds,
                           void *out, unsigned long long *counters, uint32_t grid_waves_per_simd,
                           int static_lanes, void *stream);
// The same query with material scattering (rvcp_set_materials): the queue form
// only; raw_materials is the scene's rvcp_material_t array as uploaded (fuzz, refraction_ratio).
int rvcp_launch_path_scatter(const rvcp::FrameArgs *args, const rvcp::TriRecord *tri,
                             const rvcp::FaceShade *shade, const rvcp::MatRecord *mats,
                             const void *raw_materials, const rvcp::LightRecord *lights,
                             const rvcp::Bvh4Node *bvh_nodes, const rvcp::TriRecord *bvh_tris,
                             const void *rays, const void *seeds, void *out,
                             unsigned long long *counters, uint32_t grid_waves_per_simd,
                             void *stream);
// The seeds of the first `count` pixels of args' frame, one float each (rvcp_primary_seeds_async)
int rvcp_launch_primary_seeds(const rvcp::FrameArgs *args, uint32_t count, void *out, void *stream);
// tonemap_kernel alone (the denoiser's RGBA8 store)
int rvcp_launch_tonemap(const float *lin, uint32_t n, const float *gamma_t, uint32_t *out_rgba,
                        void *stream);
// One a-trous pass (rvcp_denoise.hip): step = 2^i, color_s2 = sigma_i^2 (use_color = 0: the
// colour weight is 1)
int rvcp_launch_denoise_pass(const float *in, const void *gbuffer, float *out, uint32_t width,
                             uint32_t height, uint32_t step, uint32_t normal_power_log2,
                             uint32_t use_color, float color_s2, float sigma_plane, void *stream);
// One temporal accumulation step (rvcp_temporal.hip): mode 0 no history (prev_* unused), 1 the
// identity mapping, 2 reprojection through *view
int rvcp_launch_temporal(const float *cur_c, const void *cur_g, const float *prev_c,
                         const void *prev_g, const uint32_t *prev_len, float *out_c,
                         uint32_t *out_len, uint32_t width, uint32_t height, uint32_t mode,
                         const struct rvcp_temporal_view *view,
                         const struct rvcp_temporal_params *params, void *stream);
// SVGF (rvcp_svgf.hip): the accumulation step with moments (modes as
// rvcp_launch_temporal, whose body it shares in rvcp_temporal.hip), moments -> variance, and one variance-guided a-trous pass (step = 2^i,
// sigma_l2 = sigma_luminance^2; use_lum = 0: the luminance weight is 1; force_direct: steps 1
// and 2 through the direct kernel too)
int rvcp_launch_svgf_temporal(const float *cur_c, const void *cur_g, const float *prev_c,
                              const void *prev_g, const uint32_t *prev_len, const float *prev_m,
                              float *out_c, uint32_t *out_len, float *out_m, uint32_t width,
                              uint32_t height, uint32_t mode,
                              const struct rvcp_temporal_view *view,
                              const struct rvcp_temporal_params *params, float alpha_moments_min,
                              void *stream);
int rvcp_launch_svgf_variance(const float *moments, const uint32_t *len, const void *gbuffer,
                              float *out_v, uint32_t width, uint32_t height,
                              uint32_t spatial_below, uint32_t normal_power_log2,
                              float sigma_plane, void *stream);
int rvcp_launch_svgf_pass(const float *in_c, const float *in_v, const void *gbuffer, float *out_c,
                          float *out_v, uint32_t width, uint32_t height, uint32_t step,
                          uint32_t normal_power_log2, uint32_t use_lum, float sigma_l2,
                          float epsilon, float sigma_plane, uint32_t force_direct, void *stream);
// Albedo demodulation (rvcp_albedo.hip) over n pixels: albedo is the context's
// table of n_materials float4 (the albedo as uploaded); in == out is legal for the demodulation;
// the remodulation writes out_lin and / or out_rgba (either may be null)
int rvcp_launch_demodulate(const float *in, const void *gbuffer, const void *albedo,
                           uint32_t n_materials, float *out, uint32_t n, void *stream);
int rvcp_launch_remodulate(const float *in, const void *gbuffer, const void *albedo,
                           uint32_t n_materials, const float *gamma_t, float *out_lin,
                           uint32_t *out_rgba, uint32_t n, void *stream);
// The TAA resolve (rvcp_taa.hip): mode 0 no history (prev_* unused), 1 the
// identity mapping, 2 reprojection from *cur_view into *prev_view; out_rgba may be null
int rvcp_launch_taa_resolve(const float *cur_c, const void *cur_g, const float *prev_c,
                            const uint32_t *prev_len, float *out_c, uint32_t *out_len,
                            uint32_t *out_rgba, const float *gamma_t, uint32_t width,
                            uint32_t height, uint32_t mode,
                            const struct rvcp_temporal_view *cur_view,
                            const struct rvcp_temporal_view *prev_view,
                            const struct rvcp_taa_params *params, void *stream);
// The temporal upsampling step (rvcp_taau.hip) of a width x height OUTPUT frame
// from a frame traced at width / scale x height / scale: modes as the TAA resolve's (g_hi is read
// in mode 2 only, prev_* in modes 1 and 2); out_rgba and prev_view may be null; force_direct: the
// form without LDS staging (tools/taau_time.py's comparison)
int rvcp_launch_taa_upsample(const float *cur_c, const void *g_hi, const float *prev_c,
                             const float *prev_w, float *out_c, float *out_w, uint32_t *out_rgba,
                             const float *gamma_t, uint32_t width, uint32_t height, uint32_t scale,
                             uint32_t mode, const struct rvcp_temporal_view *jit_view,
                             const struct rvcp_temporal_view *cur_view,
                             const struct rvcp_temporal_view *prev_view,
                             const struct rvcp_taau_params *params, uint32_t force_direct,
                             void *stream);
// The plan step of adaptive sampling (rvcp_adaptive.hip) over n_pixels pixels:
// priorities into q_plane and their sum into sums[0], then the map into map_out and its sum into
// sums[1] (sums: two zeroed 64-bit words); len may be null (1 everywhere); extra = the budget
// above spp_min for every pixel.  And a uniform map of `value`.
int rvcp_launch_spp_plan(const float *var, const float *lin, const uint32_t *len,
                         const void *gbuffer, uint32_t n_pixels, float weight_cap, float epsilon,
                         uint32_t spp_min, uint32_t spp_max, unsigned long long extra,
                         uint32_t *q_plane, unsigned long long *sums, uint32_t *map_out,
                         void *stream);
int rvcp_launch_fill_map(uint32_t *map, uint32_t n_pixels, uint32_t value, void *stream);
int rvcp_launch_assemble(const uint32_t *gathered, uint32_t slot_rows, uint32_t width,
                         uint32_t height, uint32_t shard_count, uint32_t *frame, void *stream);
int rvcp_launch_fill(uint32_t *out_rgba, float *out_lin, uint32_t n_pixels, uint32_t rgba,
                     void *stream);
}
#endif  // __HIPCC_RTC__
