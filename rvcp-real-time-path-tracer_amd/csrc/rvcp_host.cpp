// rvcp_host.cpp -- C-ABI host runtime of librvcp (include/rvcp.h).
//
// Replaces the Vulkano runtime of the reference (src/ray_tracer/vulkan.rs): pipeline
// creation (:576-603) -> rvcp_create, descriptor-set upload (:454-574) -> rvcp_upload_scene,
// push constants + dispatch (:406-452) -> rvcp_render / rvcp_render_shard_async.
//
// Compiled with hipcc -ffp-contract=off: the frame constants it derives (camera basis,
// light-area prefix sums, gamma thresholds) use the same float operations as the shader, so
// the kernel's results stay bit-identical to the CPU oracle.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <exception>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rvcp.h"
#include "rvcp_internal.h"
#include "rvcp_frame_plan.h"
#include "rvcp_jit.h"
#include "rvcp_scene_prep.h"
#include "build/rvcp_build_id.h"     // kRvcpSourceHash (Makefile)

using namespace rvcp;

// The static builds of the games101 kernels, [sampling][map] (rvcp_internal.h)
const KernelBuild *const rvcp::kKernelBuilds[2][2] = {
    {&rvcp_games101_build, &rvcp_games101_map_build},
    {&rvcp_games101_cosine_build, &rvcp_games101_cosine_map_build}};

// Experiment knobs (grid caps, fixed queue grabs, small-frame spreading, per-wave timelines,
// generic-scan forcing) are read from the environment only in the debug build of the library
// (make debug -> build/librvcp_debug.so, -DRVCP_DEBUG_KNOBS, used by tools/).  The product
// library's behaviour depends on rvcp_config_t alone: here the names are not even compiled in.
#ifdef RVCP_DEBUG_KNOBS
#define RVCP_KNOB(name) std::getenv(name)
#else
#define RVCP_KNOB(name) ((const char *)nullptr)
#endif

// The specialised pre-pass (rvcp_spec_primary_kernel) with the specialised path kernels; the
// debug build's RVCP_DEBUG_GENERIC_PREPASS=1 keeps the built-in one (A/B)
static bool jit_spec_prepass()
{
    const char *e = RVCP_KNOB("RVCP_DEBUG_GENERIC_PREPASS");
    return !(e && *e == '1');
}

// rvcp_rccl_init / rvcp_gather_wait give up after this long unless rvcp_rccl_set_timeout says
// otherwise: far above a frame (C5 brute force, the slowest workload, 6.5 s) and far below
// "forever", which is what a blocking ncclCommInitRank or an unbounded event wait gives when a
// peer never arrives
constexpr uint32_t kDefaultCommTimeoutMs = 60000;

// One post-process step's bracket on its stream: ev0 / ev1 are recorded around the work of the
// step's last call (each created on first use).  recorded: ev1 has been recorded at least once
// (steps are ordered behind it, rvcp_destroy synchronises it); pending: ... and not yet waited for.
struct Stage {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool recorded = false, pending = false;
};

enum StageId {
    ST_DENOISE, ST_TEMPORAL, ST_SVGF_ACC, ST_SVGF_FLT, ST_DEMOD, ST_REMOD, ST_TAA, ST_TAAU, ST_PLAN,
    ST_RAYS, ST_RAYS_SYNC, ST_PATHS, ST_PATHS_SYNC, N_STAGES
};

constexpr uint32_t stage_bit(StageId id) { return 1u << id; }

// The steps each step is ordered behind, besides a render pending on another stream: the denoiser,
// the temporal step, the TAA resolve and the upsampling step reuse what their own previous call
// wrote (intermediates, or the history); the SVGF and the albedo steps share buffers from call to
// call, so each waits for the context's previous SVGF accumulation and filter; the plan step of
// adaptive sampling reuses its own priority plane and sums; a ray query is ordered behind the
// context's previous one, asynchronous (ST_RAYS) or synchronous (ST_RAYS_SYNC: rvcp_trace_rays and
// rvcp_pick, which bracket their query with events of their own so that they leave a pending
// rvcp_trace_rays_async to its rvcp_rays_wait); a path query likewise (ST_PATHS, and ST_PATHS_SYNC
// for rvcp_trace_paths).  (In StageId order.)
constexpr uint32_t kSvgfSteps = stage_bit(ST_SVGF_ACC) | stage_bit(ST_SVGF_FLT);
constexpr uint32_t kRaySteps = stage_bit(ST_RAYS) | stage_bit(ST_RAYS_SYNC);
constexpr uint32_t kPathSteps = stage_bit(ST_PATHS) | stage_bit(ST_PATHS_SYNC);
constexpr uint32_t kStageBehind[N_STAGES] = {
    stage_bit(ST_DENOISE), stage_bit(ST_TEMPORAL), kSvgfSteps, kSvgfSteps, kSvgfSteps, kSvgfSteps,
    stage_bit(ST_TAA), stage_bit(ST_TAAU), stage_bit(ST_PLAN), kRaySteps, kRaySteps,
    kPathSteps, kPathSteps};

// A history a stateful chain keeps from call to call, ping-ponging between slots `slot` (the
// previous frame) and slot ^ 1
struct History {
    uint32_t slot = 0, width = 0, height = 0;
    bool valid = false;                 // slot `slot` holds a frame of width x height
    rvcp_camera_t camera = {};          // ... rendered from this camera
    rvcp_temporal_view_t view = {};     // ... whose projection (at width x height) this is

    bool continues_at(uint32_t w, uint32_t h) const { return valid && width == w && height == h; }
    void commit(uint32_t w, uint32_t h, const rvcp_camera_t &c, const rvcp_temporal_view_t &v)
    {
        slot ^= 1u;
        width = w;
        height = h;
        camera = c;
        view = v;
        valid = true;
    }
};

// What a stateful chain keeps for the step that ends its frames with the TAA switch set (the
// resolve) or the upsampling scale above 1 (§4.14): the resolved colour and a
// 4-byte plane (the resolve's history lengths, the upsampling's weights) under the unjittered
// camera, and for the upsampling the output-size G-buffer of a frame whose camera moved
struct ResolveState {
    History hist;
    float *d_res[2] = {nullptr, nullptr};
    void *d_aux[2] = {nullptr, nullptr};
    void *d_gbuf = nullptr;
    size_t cap = 0;
    uint32_t counter = 0;               // the next frame's index into the jitter sequence
};


struct rvcp_ctx {
    rvcp_config_t cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, evm = nullptr, ev1 = nullptr;   // start, main kernel, end
    hipEvent_t evg0 = nullptr, evg1 = nullptr;                // gather start / end
    // rvcp_gather_frame_async without a caller stream runs on gstream (high priority), joined
    // to the render stream by events: evr (render done) before the gather, evg1 (gather done)
    // before the next render on this context overwrites the shard buffer the gather reads
    hipStream_t gstream = nullptr;
    hipStream_t render_stream = nullptr;     // the stream of the last render (the caller's or ours)
    hipEvent_t evr = nullptr;
    bool gather_on_gstream = false;
    bool gather_pending = false;
    // resident workgroups per kernel variant and of the RVCP_ACCEL_BVH path kernel, for each
    // build of the games101 kernels as kKernelBuilds indexes them: [sampling][map] (a map build
    // has schedules 3-6 and 10 only; its other slots stay 0)
    struct Capacity {
        int grid[kMaxVariant + 1] = {};
        int bvh = 0;
    } capacity[2][2];
    int legacy_capacity = 0;                   // ... of the RVCP_INTEGRATOR_LEGACY kernel
    uint32_t n_simds = 1024;

    // scene (device)
    TriRecord *d_tri = nullptr;
    rvcp_face_t *d_faces = nullptr;
    rvcp_vertex_t *d_verts = nullptr;
    MatRecord *d_mats = nullptr;
    FaceShade *d_shade = nullptr;
    LightRecord *d_lights = nullptr;
    rvcp_material_t *d_rawmats = nullptr;     // RVCP_INTEGRATOR_LEGACY: fuzz / ior needed
    rvcp_sphere_t *d_spheres = nullptr;
    // opt-in BVH (RVCP_ACCEL_BVH): nodes, leaf-ordered triangles and their face ids
    Bvh4Node *d_bvh_nodes = nullptr;
    TriRecord *d_bvh_tris = nullptr;
    int32_t bvh_root = 0;
    uint32_t bvh_n4 = 0;
    uint32_t bvh_slots = 0;
    int bvh_depth = 0;
    uint32_t bvh_prefix = 0;    // faces [0, bvh_prefix) left out of the BVH (FrameArgs::bvh_prefix)
    float *d_gamma = nullptr;
    float *d_unorm = nullptr;
    unsigned long long *d_counters = nullptr;
    uint32_t n_faces = 0, n_lights = 0, n_mats = 0, n_verts = 0, n_spheres = 0;
    bool lights_same = false;      // every light record samples the same face
    bool rcp_fast = false;         // scan_rcp_fast_scene (FrameArgs::rcp_fast)
    bool has_metal = false;        // a material of type 1 (FrameArgs::has_metal)
    // scene-specialised path kernels (rvcp_jit.cpp), or null: generic kernels.  By map: jit[0]
    // serves the default renders, jit[1] the map renders (rvcp_render_spp_map_async,
    // -DRVCP_SPP_MAP=1).
    // The default slot is compiled at upload and records its error in jit_err.
    std::shared_ptr<JitKernels> jit[2];
    std::string jit_err;
    // bounce sampling (rvcp_set_sampling).  A games101 module is compiled for
    // one mode: jit_sampling[m] is the mode jit[m] was asked for, jit_tri / jit_bvh what upload
    // asked it with (empty: the scene gets no module), so that the first render after a switch
    // can ask again for the other mode (jit_for_render).
    // The map slot is compiled by the first map render of a scene -- jit_sampling[1] is -1 before
    // any (and after an upload) -- and its error is dropped.
    int32_t sampling = RVCP_SAMPLING_UNIFORM;
    int32_t jit_sampling[2] = {RVCP_SAMPLING_UNIFORM, -1};
    std::vector<TriRecord> jit_tri;
    bool jit_bvh = false;
    uint64_t jit_lum = 0;       // the luminous faces' mask the module was asked with (JitSpec::lum_mask)
    float light_total = 0.0f, light_pdf = 0.0f;
    bool has_scene = false;

    // primary pre-pass output (variant 3): compact list of surface pixels
    SurfRecord *d_surf = nullptr;
    size_t cap_surf = 0;
    float *d_acc = nullptr;         // linear colours for tonemap_kernel when the caller wants none
    size_t cap_acc = 0;
    // mode-2 batches: the frames' FrameCam records (16 floats each), staged through pinned
    // host memory (one render in flight per context, so the staging is free again at the next)
    float *d_cams = nullptr, *h_cams = nullptr;
    uint32_t cap_cams = 0;

    // staging for the synchronous host API
    uint32_t *d_rgba = nullptr;
    float *d_lin = nullptr;
    size_t cap_rgba = 0, cap_lin = 0;
    // n_gpus > 1: shard 0's packed stripes
    uint32_t *d_pack_rgba = nullptr;
    float *d_pack_lin = nullptr;
    size_t cap_surf_pack = 0;

    // the event brackets of the post-process steps (rvcp_*_async / rvcp_*_wait), by StageId
    Stage stage[N_STAGES];

    // denoiser (rvcp_denoise_async): the passes between the first and the last ping-pong
    // between d_dn[0] and d_dn[1].  rvcp_render_denoised keeps its G-buffer and linear frames
    // here too.
    float *d_dn[2] = {nullptr, nullptr};
    size_t cap_dn[2] = {0, 0};
    void *d_gbuf = nullptr;
    float *d_dn_in = nullptr, *d_dn_out = nullptr;
    size_t cap_gbuf = 0, cap_dn_in = 0, cap_dn_out = 0;

    // rvcp_render_temporal keeps its history here: accumulated colour, history length and
    // G-buffer ping-pong between the slots of tp_hist; d_tp_cur is the raw frame, d_tp_show the
    // filtered one.
    float *d_tp_lin[2] = {nullptr, nullptr};
    uint32_t *d_tp_len[2] = {nullptr, nullptr};
    void *d_tp_gbuf[2] = {nullptr, nullptr};
    float *d_tp_cur = nullptr, *d_tp_show = nullptr;
    size_t cap_tp = 0, cap_tp_show = 0;
    History tp_hist;

    // SVGF (rvcp_svgf_accumulate_async / rvcp_svgf_filter_async): the filter's
    // variance planes (d_sv_var: the estimate and the passes' ping-pong) and colour intermediates.
    // rvcp_render_svgf keeps a history of its own, apart from rvcp_render_temporal's: colour,
    // moments, length and G-buffer ping-pong between the slots of sv_hist; d_sv_cur is the raw
    // frame, d_sv_show and d_sv_showvar the filtered one and its variance, d_sv_fb pass 0's colour
    // (feedback).
    float *d_sv_var[2] = {nullptr, nullptr}, *d_sv_tmp[2] = {nullptr, nullptr};
    size_t cap_sv_var[2] = {0, 0}, cap_sv_tmp[2] = {0, 0};
    float *d_sv_lin[2] = {nullptr, nullptr}, *d_sv_mom[2] = {nullptr, nullptr};
    uint32_t *d_sv_len[2] = {nullptr, nullptr};
    void *d_sv_gbuf[2] = {nullptr, nullptr};
    float *d_sv_cur = nullptr, *d_sv_show = nullptr, *d_sv_showvar = nullptr, *d_sv_fb = nullptr;
    size_t cap_sv = 0;
    History sv_hist;

    // adaptive sampling.  The plan step (rvcp_spp_plan_async) keeps its
    // priority plane and its two 64-bit sums (sum of priorities, sum of the map) here.  The switch
    // of rvcp_set_adaptive and its parameters; while it is set rvcp_render_svgf traces through
    // d_ad_map[ad_slot] -- the plan of its previous frame while ad_valid (and the SVGF history
    // continues), else a uniform map -- and plans the next frame into the other slot.  ad_last:
    // the slot the last such frame was traced through (-1: none yet), ad_w x ad_h its size.
    uint32_t *d_ad_q = nullptr;
    size_t cap_ad_q = 0;
    unsigned long long *d_ad_sums = nullptr;
    bool adaptive = false;
    rvcp_adaptive_params_t ad_params = {};
    uint32_t *d_ad_map[2] = {nullptr, nullptr};
    size_t cap_ad_map[2] = {0, 0};
    uint32_t ad_slot = 0, ad_w = 0, ad_h = 0;
    int ad_last = -1;
    bool ad_valid = false;

    // ray queries: the staging of the synchronous rvcp_trace_rays and rvcp_pick
    void *d_q_rays = nullptr, *d_q_out = nullptr;
    size_t cap_q_rays = 0, cap_q_out = 0;

    // path queries: the staging of the synchronous rvcp_trace_paths, and the
    // queries' own counter words (kPathCounterWords for ST_PATHS, then as many for ST_PATHS_SYNC:
    // traversals, queue head, wave iterations), apart from the render's d_counters
    void *d_p_rays = nullptr, *d_p_seeds = nullptr, *d_p_out = nullptr;
    size_t cap_p_rays = 0, cap_p_seeds = 0, cap_p_out = 0;
    unsigned long long *d_p_counters = nullptr;

    // material scattering (rvcp_set_materials): the mode, the scene's materials
    // as uploaded (the mode's validation reads fuzz and refraction_ratio when it is switched on
    // after an upload) and the frame route's primary rays and seeds
    int32_t materials = RVCP_MATERIALS_LAMBERTIAN;
    std::vector<rvcp_material_t> h_rawmats;
    void *d_ms_rays = nullptr, *d_ms_seeds = nullptr;
    size_t cap_ms_rays = 0, cap_ms_seeds = 0;
    bool last_scatter = false;      // the last render took that route: its kernel counts every
                                    // traversal, the kept first hit's included

    // albedo demodulation (rvcp_demodulate_async / rvcp_remodulate_async): the
    // scene's albedo table (one float4 per material, made by every upload) and the switch of
    // rvcp_set_demodulation: while it is set rvcp_render_denoised, rvcp_render_temporal and
    // rvcp_render_svgf filter irradiance
    float *d_albedo = nullptr;
    bool demodulation = false;

    // temporal anti-aliasing and temporal upsampling (§4.14): the switch of
    // rvcp_set_taa, the scale of rvcp_set_taa_upsample (1: off), and for each of the two one
    // state per stateful chain (of rvcp_render_temporal / rvcp_render_svgf); the upsampling's is
    // at the OUTPUT size
    bool taa = false;
    uint32_t taau_scale = 1;
    ResolveState taa_tp, taa_sv, taau_tp, taau_sv;

    // debug build: per-wave timeline of the path kernel appended per render
    unsigned long long *d_timeline = nullptr;
    size_t cap_timeline = 0, last_timeline_waves = 0;

    // n_gpus > 1: contexts of the other GPUs (shards 1..N-1) and their packed shard buffers
    std::vector<rvcp_ctx *> subs;
    std::vector<uint32_t *> shard_rgba;
    std::vector<float *> shard_lin;
    std::vector<size_t> shard_cap;

    // one process per GPU: the RCCL communicator of rvcp_gather_frame_async (rank `comm_rank`
    // of `comm_world`; created by rvcp_rccl_init, or the caller's by rvcp_rccl_attach)
    ncclComm_t comm = nullptr;
    bool comm_owned = false;
    uint32_t comm_world = 0, comm_rank = 0;
    // deadline of rvcp_rccl_init and rvcp_gather_wait (rvcp_rccl_set_timeout; 0 = none)
    uint32_t comm_timeout_ms = kDefaultCommTimeoutMs;
    // the last communicator was given up after a deadline: gathers return RVCP_E_TIMEOUT (not
    // "no communicator") until rvcp_rccl_init / rvcp_rccl_attach provides a new one
    bool comm_timed_out = false;
    // the creation worker of an rvcp_rccl_init that timed out, while it is still blocked inside
    // RCCL: a further rvcp_rccl_init on this context is refused (RVCP_E_BUSY) until it returns,
    // so retries cannot pile up blocked threads and half-made communicators
    std::shared_ptr<struct CommJob> init_job;
    // detached ncclCommAbort calls of this context's communicators (abort_comm): rvcp_destroy
    // waits for them (bounded) before it frees the buffers and streams their kernels used
    std::vector<std::shared_ptr<std::atomic<bool>>> aborts;
    // end events of gathers that timed out and whose stream did not drain (a collective on an
    // attached communicator, which only its owner can abort): renders no longer wait for them,
    // the gather stream they sit on is retired, and rvcp_destroy checks them before freeing
    // device memory (HIP's hipFree synchronises the whole device)
    std::vector<hipEvent_t> stuck_gathers;
    std::vector<hipStream_t> retired_gstreams;

    // last launch
    bool pending = false;
    bool last_trivial = false;
    int32_t last_variant = 0;
    uint64_t last_pixels = 0;
    uint32_t last_spp = 0;
    bool last_map = false;          // the last render was a map render: its counts are the pre-pass's sum
    uint32_t last_shard_index = 0, last_shard_count = 0;   // of the last rvcp_render_shard_async
    uint32_t last_width = 0, last_height = 0;

    std::string err;
};

namespace {

thread_local std::string g_create_error;

int fail(rvcp_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}

// RCCL, resolved at run time: dlopen("librccl.so.1") returns the copy the process already
// holds (PyTorch-ROCm's, soname librccl.so.1, or the host's own) and otherwise the system one,
// so librvcp needs no RCCL to load and shares one RCCL with its host.
struct RcclApi {
    ncclResult_t (*get_unique_id)(ncclUniqueId *) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    // non-blocking creation, abort and the communicator's asynchronous state: what makes a
    // missing or failed peer a timeout instead of a hang (rccl.h: ncclCommInitRankConfig,
    // ncclCommAbort, ncclCommGetAsyncError; present in every RCCL >= 2.14)
    ncclResult_t (*comm_init_rank_config)(ncclComm_t *, int, ncclUniqueId, int, ncclConfig_t *) = nullptr;
    ncclResult_t (*comm_abort)(ncclComm_t) = nullptr;
    ncclResult_t (*get_async_error)(ncclComm_t, ncclResult_t *) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*gather)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t,
                           hipStream_t) = nullptr;
    const char *(*error_string)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};

const RcclApi &rccl_api()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char *e = dlerror();
            api.why = std::string("cannot load librccl.so.1: ") + (e ? e : "?");
            return;
        }
        api.get_unique_id = (decltype(api.get_unique_id))dlsym(h, "ncclGetUniqueId");
        api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(h, "ncclCommInitRank");
        api.comm_init_rank_config = (decltype(api.comm_init_rank_config))dlsym(h, "ncclCommInitRankConfig");
        api.comm_abort = (decltype(api.comm_abort))dlsym(h, "ncclCommAbort");
        api.get_async_error = (decltype(api.get_async_error))dlsym(h, "ncclCommGetAsyncError");
        api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
        api.gather = (decltype(api.gather))dlsym(h, "ncclGather");
        api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
        api.ok = api.get_unique_id && api.comm_init_rank && api.comm_init_rank_config &&
                 api.comm_abort && api.get_async_error && api.comm_destroy && api.gather &&
                 api.error_string;
        if (!api.ok)
            api.why = "librccl.so.1 lacks ncclGather / ncclCommInitRankConfig / ncclCommAbort / "
                      "ncclCommGetAsyncError";
    });
    return api;
}

// Report an error without allocating on the failure path that may itself be out of memory.
int fail_noexcept(rvcp_ctx *ctx, int code, const char *msg) noexcept
{
    try {
        if (ctx) ctx->err = msg;
        else g_create_error = msg;
    } catch (...) {
    }
    return code;
}

template <typename F>
int barrier(rvcp_ctx *ctx, F &&f) noexcept
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail_noexcept(ctx, RVCP_E_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return fail_noexcept(ctx, RVCP_E_INTERNAL, e.what());
    } catch (...) {
        return fail_noexcept(ctx, RVCP_E_INTERNAL, "unknown C++ exception");
    }
}

#define HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail((ctx), RVCP_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// sample_ray's frame constants, :217-227
void camera_constants(const rvcp_push_constant_t &pc, uint32_t W, uint32_t H, FrameArgs &A)
{
    const float PI = 3.1415926f;
    h3 cpos = ld3h(pc.camera.position), up = ld3h(pc.camera.up), fwd = ld3h(pc.camera.forward);
    const float rad = pc.camera.vertical_fov / 2.0f * PI / 180.0f;   // degree_to_radian :141
    const float h = 2.0f * pc.camera.t_near * std::tan(rad);
    const float w = h * (float)W / (float)H;
    h3 u = muls(normalize(cross(fwd, up)), w);
    h3 v = muls(normalize(cross(fwd, u)), h);
    h3 pos = add(cpos, muls(fwd, pc.camera.t_near));
    st3(A.cam_pos, cpos);
    st3(A.u, u);
    st3(A.v, v);
    st3(A.pos, pos);
    A.base_len = length(sub(pos, cpos));
    A.t_near = pc.camera.t_near;
    A.t_far = pc.camera.t_far;
    A.time = pc.time;
}

// One frame's FrameCam record, the 16 floats a batch's kernels read per frame
// (FrameArgs::batch_cams, the batched pre-pass): cam_pos, u, v, pos, base_len, t_near, t_far, time
void pack_frame_cam(const FrameArgs &A, float *c)
{
    std::memcpy(c, A.cam_pos, 12);
    std::memcpy(c + 3, A.u, 12);
    std::memcpy(c + 6, A.v, 12);
    std::memcpy(c + 9, A.pos, 12);
    c[12] = A.base_len;
    c[13] = A.t_near;
    c[14] = A.t_far;
    c[15] = A.time;
}

// The fields of FrameArgs the primary ray and its scan read: the camera, the frame's size, the
// face count and the BVH (render_frames, rvcp_render_gbuffer_async)
void primary_frame_args(const rvcp_ctx *ctx, const rvcp_push_constant_t &pc, uint32_t W, uint32_t H,
                        FrameArgs &A)
{
    camera_constants(pc, W, H, A);
    A.width = W;
    A.height = H;
    A.n_faces = ctx->n_faces;
    A.accel = resolved_accel(ctx->cfg.accel, ctx->n_faces);
    A.bvh_root = ctx->bvh_root;
    A.bvh_n4 = ctx->bvh_n4;
    A.bvh_slots = ctx->bvh_slots;
    A.bvh_prefix = A.accel == RVCP_ACCEL_BVH ? ctx->bvh_prefix : 0u;
}

// The primary ray's range is [t_near, t_far] x t_coef (sample_ray, :226-233), and a miss is
// written as t_max + 1 (:287) and detected as t > t_max (:424): once t_max reaches 2^24 the +1
// is lost and the shader takes a miss for a hit on uninitialised data.  The kernels detect a
// miss by the absent face instead, so such a frame would differ from the reference's; it is
// refused, as rvcp_config_t.ray_t_max >= 2^24 is for the secondary rays.  t_coef is at most
// |corner of the image plane - eye| / t_near = sqrt(1 + tan^2(fov / 2) (1 + (W / H)^2))
// (u, v, forward orthogonal); a 1e-3 margin covers the float rounding of the shader's t_coef.
bool primary_t_range_ok(const rvcp_push_constant_t &pc, uint32_t W, uint32_t H)
{
    const double tf = pc.camera.t_far;
    const double t = std::tan((double)pc.camera.vertical_fov / 2.0 * 3.1415926 / 180.0);
    const double a = (double)W / (double)H;
    const double tc = std::sqrt(1.0 + t * t * (1.0 + a * a));
    return std::fabs(tf) * tc * (1.0 + 1e-3) < 16777216.0;
}

template <typename T>
int dev_upload(rvcp_ctx *ctx, T **dst, const void *src, size_t n)
{
    if (*dst) { (void)hipFree(*dst); *dst = nullptr; }
    const size_t bytes = n ? n * sizeof(T) : sizeof(T);
    HIP_TRY(ctx, hipMalloc((void **)dst, bytes));
    if (n) HIP_TRY(ctx, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return RVCP_OK;
}

// *buf holds at least n elements of `elem` bytes: a buffer too small is freed and allocated anew
int grow(rvcp_ctx *ctx, void **buf, size_t *cap, size_t n, size_t elem)
{
    if (*cap >= n) return RVCP_OK;
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    HIP_TRY(ctx, hipMalloc(buf, n * elem));
    *cap = n;
    return RVCP_OK;
}

// ... a batch's n FrameCam records (64 B each): the device buffer and its pinned staging
int grow_cams(rvcp_ctx *ctx, uint32_t n)
{
    if (ctx->cap_cams >= n) return RVCP_OK;
    (void)hipFree(ctx->d_cams);
    (void)hipHostFree(ctx->h_cams);
    ctx->d_cams = ctx->h_cams = nullptr;
    ctx->cap_cams = 0;
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_cams, (size_t)n * 64));
    HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_cams, (size_t)n * 64));
    ctx->cap_cams = n;
    return RVCP_OK;
}

// ... a packed shard's bytes and linear colours on `device` (render_multi), px pixels each and one
// pixel of slack; both are made anew when the linear buffer is wanted and missing
int grow_packed(rvcp_ctx *ctx, int device, uint32_t **rgba, float **lin, size_t *cap, size_t px,
                bool want_lin)
{
    if (*cap >= px && !(want_lin && !*lin)) return RVCP_OK;
    HIP_TRY(ctx, hipSetDevice(device));
    (void)hipFree(*rgba);
    (void)hipFree(*lin);
    *rgba = nullptr;
    *lin = nullptr;
    *cap = 0;
    HIP_TRY(ctx, hipMalloc((void **)rgba, px * 4 + 4));
    HIP_TRY(ctx, hipMalloc((void **)lin, px * 12 + 12));
    *cap = px;
    return RVCP_OK;
}

void free_scene(rvcp_ctx *ctx)
{
    (void)hipFree(ctx->d_tri); ctx->d_tri = nullptr;
    (void)hipFree(ctx->d_faces); ctx->d_faces = nullptr;
    (void)hipFree(ctx->d_verts); ctx->d_verts = nullptr;
    (void)hipFree(ctx->d_mats); ctx->d_mats = nullptr;
    (void)hipFree(ctx->d_shade); ctx->d_shade = nullptr;
    (void)hipFree(ctx->d_lights); ctx->d_lights = nullptr;
    (void)hipFree(ctx->d_rawmats); ctx->d_rawmats = nullptr;
    (void)hipFree(ctx->d_albedo); ctx->d_albedo = nullptr;
    (void)hipFree(ctx->d_spheres); ctx->d_spheres = nullptr;
    (void)hipFree(ctx->d_bvh_nodes); ctx->d_bvh_nodes = nullptr;
    (void)hipFree(ctx->d_bvh_tris); ctx->d_bvh_tris = nullptr;
    ctx->jit[0].reset();
    ctx->jit[1].reset();
    ctx->jit_sampling[1] = -1;
    ctx->has_scene = false;
}

// The buffer groups of the stateful chains.  Each has one function that frees it and one that
// makes it hold npx pixels: a larger frame drops the history with its buffers.
template <typename T>
void dev_free(T *&p)
{
    (void)hipFree(p);
    p = nullptr;
}

void free_temporal_state(rvcp_ctx *ctx)
{
    for (int i = 0; i < 2; ++i) {
        dev_free(ctx->d_tp_lin[i]);
        dev_free(ctx->d_tp_len[i]);
        dev_free(ctx->d_tp_gbuf[i]);
    }
    dev_free(ctx->d_tp_cur);
    ctx->cap_tp = 0;
}

int reserve_temporal_state(rvcp_ctx *ctx, size_t npx)
{
    if (ctx->cap_tp >= npx) return RVCP_OK;
    ctx->tp_hist.valid = false;
    free_temporal_state(ctx);
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_tp_lin[i], npx * 12));
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_tp_len[i], npx * 4));
        HIP_TRY(ctx, hipMalloc(&ctx->d_tp_gbuf[i], npx * sizeof(rvcp_gbuffer_texel_t)));
    }
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_tp_cur, npx * 12));
    ctx->cap_tp = npx;
    return RVCP_OK;
}

void free_svgf_state(rvcp_ctx *ctx)
{
    for (int i = 0; i < 2; ++i) {
        dev_free(ctx->d_sv_lin[i]);
        dev_free(ctx->d_sv_mom[i]);
        dev_free(ctx->d_sv_len[i]);
        dev_free(ctx->d_sv_gbuf[i]);
    }
    dev_free(ctx->d_sv_cur);
    dev_free(ctx->d_sv_show);
    dev_free(ctx->d_sv_showvar);
    dev_free(ctx->d_sv_fb);
    ctx->cap_sv = 0;
}

int reserve_svgf_state(rvcp_ctx *ctx, size_t npx)
{
    if (ctx->cap_sv >= npx) return RVCP_OK;
    ctx->sv_hist.valid = false;
    free_svgf_state(ctx);
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_lin[i], npx * 12));
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_mom[i], npx * 8));
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_len[i], npx * 4));
        HIP_TRY(ctx, hipMalloc(&ctx->d_sv_gbuf[i], npx * sizeof(rvcp_gbuffer_texel_t)));
    }
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_cur, npx * 12));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_show, npx * 12));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_showvar, npx * 4));
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_sv_fb, npx * 12));
    ctx->cap_sv = npx;
    return RVCP_OK;
}

void free_resolve_state(ResolveState &st)
{
    for (int i = 0; i < 2; ++i) {
        dev_free(st.d_res[i]);
        dev_free(st.d_aux[i]);
    }
    dev_free(st.d_gbuf);
    st.cap = 0;
}

// (with_gbuf: the upsampling's output-size G-buffer)
int reserve_resolve_state(rvcp_ctx *ctx, ResolveState &st, size_t npx, bool with_gbuf)
{
    if (st.cap >= npx) return RVCP_OK;
    st.hist.valid = false;
    free_resolve_state(st);
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(ctx, hipMalloc((void **)&st.d_res[i], npx * 12));
        HIP_TRY(ctx, hipMalloc(&st.d_aux[i], npx * 4));
    }
    if (with_gbuf) HIP_TRY(ctx, hipMalloc(&st.d_gbuf, npx * sizeof(rvcp_gbuffer_texel_t)));
    st.cap = npx;
    return RVCP_OK;
}

}  // namespace

using Clock = std::chrono::steady_clock;
static void abort_comm(rvcp_ctx_t *ctx);
static int wait_gather_done(rvcp_ctx_t *ctx);

extern "C" {

// 0.2.0: ABI revision 2 (rvcp.h RVCP_ABI_VERSION: rvcp_stats_t is 64 B)
const char *rvcp_version(void) { return "rvcp-mi355x 0.3.0 (gfx950, ABI 2)"; }

uint32_t rvcp_abi_version(void) { return RVCP_ABI_VERSION; }

// Self-test / measurement hooks (not part of rvcp.h): the library's source identity (SHA-256
// prefix of every source it is built from, "+debug" for the knob build) and the key of the
// scene-specialised module ctx's last upload built (0: none) -- bench.py binds the committed
// PMC summaries to both.
const char *rvcp_internal_build_id(void)
{
#ifdef RVCP_DEBUG_KNOBS
    static const std::string id = std::string(kRvcpSourceHash) + "+debug";
    return id.c_str();
#else
    return kRvcpSourceHash;
#endif
}

uint64_t rvcp_internal_module_key(const rvcp_ctx_t *ctx)
{
    return (ctx && ctx->jit[0]) ? ctx->jit[0]->key_hash : 0;
}

static int impl_config_default_for(int32_t integrator, rvcp_config_t *cfg)
{
    if (!cfg) return RVCP_E_INVALID;
    if (integrator == RVCP_INTEGRATOR_GAMES101) return rvcp_config_default(cfg);
    if (integrator != RVCP_INTEGRATOR_LEGACY) return RVCP_E_UNSUPPORTED;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->integrator = RVCP_INTEGRATOR_LEGACY;
    cfg->spp = 5;                       // ray_tracer.comp:8
    cfg->max_bounces = 3;               // :9
    cfg->attenuation_stop_eps = 0.01f;  // :10 (unused by ray_trace)
    cfg->ray_t_min = 0.01f;             // :11
    cfg->ray_t_max = 1000.0f;           // :12
    cfg->rr_probability = 1.0f;         // :13
    cfg->eps = 0.001f;                  // :5
    cfg->lum_id_std140_quirk = 1;       // (unused by ray_trace)
    cfg->n_gpus = 1;
    return RVCP_OK;
}

static int impl_config_default(rvcp_config_t *cfg)
{
    if (!cfg) return RVCP_E_INVALID;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0;
    cfg->integrator = RVCP_INTEGRATOR_GAMES101;
    cfg->spp = 20;                      // ray_tracer_games101_branch.comp:8
    cfg->max_bounces = 15;              // :9
    cfg->attenuation_stop_eps = 0.05f;  // :10
    cfg->ray_t_min = 0.01f;             // :11
    cfg->ray_t_max = 10000.0f;          // :12
    cfg->rr_probability = 0.8f;         // :13
    cfg->eps = 0.001f;                  // :5
    cfg->lum_id_std140_quirk = 1;
    cfg->n_gpus = 1;
    return RVCP_OK;
}

const char *rvcp_last_error(const rvcp_ctx_t *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

static int impl_create(const rvcp_config_t *cfg, rvcp_ctx_t **out_ctx)
{
    if (!cfg || !out_ctx) return fail(nullptr, RVCP_E_INVALID, "null argument");
    *out_ctx = nullptr;
    if (cfg->integrator != RVCP_INTEGRATOR_GAMES101 && cfg->integrator != RVCP_INTEGRATOR_LEGACY)
        return fail(nullptr, RVCP_E_UNSUPPORTED, "unsupported integrator");
    if (cfg->spp == 0) return fail(nullptr, RVCP_E_INVALID, "spp must be > 0");
    if (cfg->kernel_variant < 0 || cfg->kernel_variant > kMaxVariant || cfg->kernel_variant == 7 ||
        cfg->kernel_variant == 8 || cfg->kernel_variant == 9)
        return fail(nullptr, RVCP_E_INVALID, "unknown kernel_variant");
    if (cfg->n_gpus < 0 || cfg->n_gpus > 64)
        return fail(nullptr, RVCP_E_INVALID, "n_gpus must be in [0, 64]");
    if (cfg->specialize != RVCP_SPECIALIZE_AUTO && cfg->specialize != RVCP_SPECIALIZE_OFF)
        return fail(nullptr, RVCP_E_INVALID, "unknown specialize");
    if (cfg->unorm_rule != RVCP_UNORM_DRIVER && cfg->unorm_rule != RVCP_UNORM_NEAREST)
        return fail(nullptr, RVCP_E_INVALID, "unknown unorm_rule");
    if (cfg->accel != RVCP_ACCEL_NONE && cfg->accel != RVCP_ACCEL_BVH)
        return fail(nullptr, RVCP_E_INVALID, "unknown accel");
    if (cfg->accel == RVCP_ACCEL_BVH && cfg->integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(nullptr, RVCP_E_UNSUPPORTED, "RVCP_ACCEL_BVH is implemented for the games101 integrator");
    if (!(cfg->ray_t_max < 16777216.0f))
        return fail(nullptr, RVCP_E_INVALID, "ray_t_max must be < 2^24 (miss test t_max + 1)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RVCP_E_HIP, "no HIP device");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, RVCP_E_INVALID, "device ordinal out of range");

    rvcp_ctx *ctx = new (std::nothrow) rvcp_ctx();
    if (!ctx) return fail(nullptr, RVCP_E_NOMEM, "out of memory");
    try {
    ctx->cfg = *cfg;
    ctx->device = cfg->device;
    auto bail = [&](int rc) {
        g_create_error = ctx->err;
        rvcp_destroy(ctx);
        return rc;
    };
    int rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return bail(fail(ctx, RVCP_E_HIP, "hipSetDevice"));
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->evm) != hipSuccess ||
        hipEventCreate(&ctx->ev1) != hipSuccess || hipEventCreate(&ctx->evg0) != hipSuccess ||
        hipEventCreate(&ctx->evg1) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->evr, hipEventDisableTiming) != hipSuccess)
        return bail(fail(ctx, RVCP_E_HIP, "stream/event creation failed"));
    // (the frame gather's own stream is created by the first gather that needs it: a context
    // that never gathers holds one stream, so the hardware queues -- GPU_MAX_HW_QUEUES, 4 by
    // default -- stay free for other contexts' render streams; frames in flight on contexts
    // whose streams shared a queue would run one after another)

    // UNORM8 thresholds on the stored value g: u8 >= k  <=>  g >= G[k].
    // RVCP_UNORM_DRIVER: u8 = (floor(4096 g) * 255 + 2048) >> 12, so G[k] = m_k / 4096 with
    // m_k = ceil((4096 k - 2048) / 255) (exact in float); RVCP_UNORM_NEAREST: G[k] = (k - 1/2) / 255.
    // Gamma thresholds on the linear colour: T[k] = float(G[k]^(1/0.6)) (pow(c, 0.6), :498).
    double G[256];
    for (int k = 1; k < 256; k++)
        G[k] = cfg->unorm_rule == RVCP_UNORM_NEAREST ? (k - 0.5) / 255.0
                                                     : std::ceil((4096.0 * k - 2048.0) / 255.0) / 4096.0;
    float T[257];
    T[0] = 0.0f;
    for (int k = 1; k < 256; k++) T[k] = (float)std::pow(G[k], 1.0 / 0.6);
    T[256] = INFINITY;
    if ((rc = dev_upload<float>(ctx, &ctx->d_gamma, T, 257)) != RVCP_OK) return bail(rc);
    // the gamma-free store of ray_tracer.comp:820-822 and mandelbrot.comp:32-33
    for (int k = 1; k < 256; k++) T[k] = (float)G[k];
    if ((rc = dev_upload<float>(ctx, &ctx->d_unorm, T, 257)) != RVCP_OK) return bail(rc);
    if (hipMalloc((void **)&ctx->d_counters, kCounterWords * sizeof(unsigned long long)) != hipSuccess)
        return bail(fail(ctx, RVCP_E_HIP, "hipMalloc counters"));

    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess)
        cus = 256;
    // debug build: cap on the persistent grid (occupancy experiments only)
    const char *cap_env = RVCP_KNOB("RVCP_DEBUG_BLOCKS_PER_CU");
    const int cap = cap_env ? std::atoi(cap_env) : 0;
    ctx->n_simds = (uint32_t)cus * 4u;
    // resident workgroups of a kernel: its occupancy per CU (1 when the query fails), capped
    auto capacity = [&](auto &&occupancy) {
        int per_cu = 0;
        if (occupancy(&per_cu) != 0 || per_cu <= 0) per_cu = 1;
        if (cap > 0 && cap < per_cu) per_cu = cap;
        return per_cu * cus;
    };
    for (int sampling = 0; sampling < 2; sampling++)
        for (int map = 0; map < 2; map++) {
            const KernelBuild &build = *kKernelBuilds[sampling][map];
            rvcp_ctx::Capacity &c = ctx->capacity[sampling][map];
            for (int v = map ? 3 : 1; v <= kMaxVariant; v++) {   // (a map build: the pre-pass schedules only)
                if (v == 7 || v == 8 || v == 9) continue;
                c.grid[v] = capacity([&build, v](int *n) { return build.occupancy(v, n); });
            }
            c.bvh = capacity([&build](int *n) { return build.occupancy(kOccupancyBvh, n); });
        }
    ctx->legacy_capacity = capacity(rvcp_legacy_occupancy);
    if (cfg->n_gpus > 1) {   // one sub-context per further GPU (shards 1..N-1)
        for (int i = 1; i < cfg->n_gpus; i++) {
            rvcp_config_t sub_cfg = *cfg;
            sub_cfg.n_gpus = 1;
            sub_cfg.device = (cfg->device + i) % ndev;
            rvcp_ctx_t *sub = nullptr;
            if ((rc = rvcp_create(&sub_cfg, &sub)) != RVCP_OK) {
                ctx->err = "sub-context on device " + std::to_string(sub_cfg.device) + ": " + g_create_error;
                return bail(rc);
            }
            ctx->subs.push_back(sub);
            ctx->shard_rgba.push_back(nullptr);
            ctx->shard_lin.push_back(nullptr);
            ctx->shard_cap.push_back(0);
            if (sub_cfg.device != cfg->device) {   // direct xGMI copies into the frame's GPU
                int ok = 0;
                if (hipDeviceCanAccessPeer(&ok, cfg->device, sub_cfg.device) == hipSuccess && ok) {
                    (void)hipSetDevice(cfg->device);
                    const hipError_t pe = hipDeviceEnablePeerAccess(sub_cfg.device, 0);
                    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                        return bail(fail(ctx, RVCP_E_HIP, "hipDeviceEnablePeerAccess failed"));
                    (void)hipGetLastError();
                }
            }
        }
        (void)hipSetDevice(cfg->device);
    }
    } catch (...) {     // the exception barrier reports it; free what was built
        rvcp_destroy(ctx);
        throw;
    }
    *out_ctx = ctx;
    return RVCP_OK;
}

static int impl_destroy(rvcp_ctx_t *ctx)
{
    if (!ctx) return RVCP_OK;
    for (size_t i = 0; i < ctx->subs.size(); i++) {
        if (!ctx->subs[i]) continue;
        (void)hipSetDevice(ctx->subs[i]->device);
        (void)hipFree(ctx->shard_rgba[i]);
        (void)hipFree(ctx->shard_lin[i]);
        rvcp_destroy(ctx->subs[i]);
    }
    ctx->subs.clear();
    (void)hipSetDevice(ctx->device);
    // a frame still in flight (possibly on the caller's stream) reads the buffers freed below
    if (ctx->pending && ctx->ev1) (void)hipEventSynchronize(ctx->ev1);
    // (a gather still pending is waited for with the deadline: a peer that never came must not
    // hang the destroy; on expiry the communicator is aborted)
    if (ctx->gather_pending && ctx->evg1 && wait_gather_done(ctx) == RVCP_OK)
        ctx->gather_pending = false;
    if (ctx->gather_pending) abort_comm(ctx);
    // the detached aborts must have returned before their communicators' buffers and streams
    // go; and a gather that never drained still reads this context's buffers, while any hipFree
    // would wait for it (HIP synchronises the device): both bounded by the deadline
    const Clock::time_point deadline = Clock::now() + std::chrono::milliseconds(
        ctx->comm_timeout_ms ? std::min<uint32_t>(ctx->comm_timeout_ms, 10000u) : 10000u);
    bool stuck = false;
    for (;;) {
        stuck = false;
        for (const auto &a : ctx->aborts) stuck |= !a->load();
        for (hipEvent_t e : ctx->stuck_gathers) stuck |= hipEventQuery(e) == hipErrorNotReady;
        if (!stuck || Clock::now() >= deadline) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (stuck) {
        // leak the device side rather than hang: the streams, events, buffers and modules stay
        // allocated for the life of the process (the owner of the attached communicator can
        // still abort it); the host side is freed
        g_create_error = "rvcp_destroy: a gather (or its communicator's abort) is still stuck "
                         "after the deadline; the context's device memory and streams are leaked";
        new std::shared_ptr<JitKernels>(std::move(ctx->jit[0]));   // never unloaded
        new std::shared_ptr<JitKernels>(std::move(ctx->jit[1]));
        delete ctx;
        return RVCP_E_TIMEOUT;
    }
    // a filter still in flight (possibly on the caller's stream) reads the buffers freed below
    for (const Stage &st : ctx->stage)
        if (st.recorded) (void)hipEventSynchronize(st.ev1);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm && ctx->comm_owned) (void)rccl_api().comm_destroy(ctx->comm);
    ctx->comm = nullptr;
    for (hipEvent_t e : ctx->stuck_gathers) (void)hipEventDestroy(e);
    for (hipStream_t s : ctx->retired_gstreams) (void)hipStreamDestroy(s);
    free_scene(ctx);
    (void)hipFree(ctx->d_gamma);
    (void)hipFree(ctx->d_unorm);
    (void)hipFree(ctx->d_counters);
    (void)hipFree(ctx->d_rgba);
    (void)hipFree(ctx->d_lin);
    (void)hipFree(ctx->d_surf);
    (void)hipFree(ctx->d_acc);
    (void)hipFree(ctx->d_cams);
    (void)hipHostFree(ctx->h_cams);
    (void)hipFree(ctx->d_timeline);
    (void)hipFree(ctx->d_pack_rgba);
    (void)hipFree(ctx->d_pack_lin);
    (void)hipFree(ctx->d_dn[0]);
    (void)hipFree(ctx->d_dn[1]);
    (void)hipFree(ctx->d_gbuf);
    (void)hipFree(ctx->d_dn_in);
    (void)hipFree(ctx->d_dn_out);
    free_temporal_state(ctx);
    (void)hipFree(ctx->d_tp_show);
    for (int i = 0; i < 2; ++i) {
        (void)hipFree(ctx->d_sv_var[i]);
        (void)hipFree(ctx->d_sv_tmp[i]);
    }
    free_svgf_state(ctx);
    (void)hipFree(ctx->d_q_rays);
    (void)hipFree(ctx->d_q_out);
    (void)hipFree(ctx->d_ms_rays);
    (void)hipFree(ctx->d_ms_seeds);
    (void)hipFree(ctx->d_p_rays);
    (void)hipFree(ctx->d_p_seeds);
    (void)hipFree(ctx->d_p_out);
    (void)hipFree(ctx->d_p_counters);
    (void)hipFree(ctx->d_ad_q);
    (void)hipFree(ctx->d_ad_sums);
    (void)hipFree(ctx->d_ad_map[0]);
    (void)hipFree(ctx->d_ad_map[1]);
    for (ResolveState *st : {&ctx->taa_tp, &ctx->taa_sv, &ctx->taau_tp, &ctx->taau_sv})
        free_resolve_state(*st);
    for (const Stage &st : ctx->stage) {
        if (st.ev0) (void)hipEventDestroy(st.ev0);
        if (st.ev1) (void)hipEventDestroy(st.ev1);
    }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->evm) (void)hipEventDestroy(ctx->evm);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->evg0) (void)hipEventDestroy(ctx->evg0);
    if (ctx->evg1) (void)hipEventDestroy(ctx->evg1);
    if (ctx->evr) (void)hipEventDestroy(ctx->evr);
    if (ctx->gstream) (void)hipStreamDestroy(ctx->gstream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return RVCP_OK;
}

static int upload_one(rvcp_ctx_t *ctx, const rvcp_material_t *materials, uint32_t n_materials,
                      const rvcp_vertex_t *vertices, uint32_t n_vertices,
                      const rvcp_face_t *faces, uint32_t n_faces,
                      const rvcp_sphere_t *spheres, uint32_t n_spheres,
                      const uint32_t *lum_face_ids, uint32_t n_lum_face_ids,
                      const uint32_t *lum_sphere_ids, uint32_t n_lum_sphere_ids);

static int impl_upload_scene(rvcp_ctx_t *ctx, const rvcp_material_t *materials, uint32_t n_materials,
                      const rvcp_vertex_t *vertices, uint32_t n_vertices,
                      const rvcp_face_t *faces, uint32_t n_faces,
                      const rvcp_sphere_t *spheres, uint32_t n_spheres,
                      const uint32_t *lum_face_ids, uint32_t n_lum_face_ids,
                      const uint32_t *lum_sphere_ids, uint32_t n_lum_sphere_ids)
{
    if (!ctx) return RVCP_E_INVALID;
    ctx->tp_hist.valid = false;     // rvcp_render_temporal: another scene, no history
    ctx->sv_hist.valid = false;     // rvcp_render_svgf likewise
    int rc = upload_one(ctx, materials, n_materials, vertices, n_vertices, faces, n_faces,
                        spheres, n_spheres, lum_face_ids, n_lum_face_ids, lum_sphere_ids,
                        n_lum_sphere_ids);
    for (rvcp_ctx *sub : ctx->subs) {
        if (rc != RVCP_OK) break;
        rc = upload_one(sub, materials, n_materials, vertices, n_vertices, faces, n_faces,
                        spheres, n_spheres, lum_face_ids, n_lum_face_ids, lum_sphere_ids,
                        n_lum_sphere_ids);
        if (rc != RVCP_OK) ctx->err = "sub-context upload: " + sub->err;
    }
    (void)hipSetDevice(ctx->device);
    return rc;
}

// What RVCP_MATERIALS_SCATTER asks of a scene's materials: a finite fuzz in
// [0, 1] for every Metal (the reference asserts fuzz <= 1, material.rs:52) and a finite
// refraction_ratio > 0 for every Dielectric; `why` names the first material that breaks it.
static bool scatter_materials_ok(const rvcp_material_t *materials, uint32_t n_materials,
                                 std::string &why)
{
    for (uint32_t i = 0; i < n_materials; i++) {
        const rvcp_material_t &m = materials[i];
        if (m.ty == 1u && !(m.fuzz >= 0.0f && m.fuzz <= 1.0f)) {
            why = "RVCP_MATERIALS_SCATTER: material " + std::to_string(i) +
                  " (Metal) needs a finite fuzz in [0, 1]";
            return false;
        }
        if (m.ty == 2u && !(m.refraction_ratio > 0.0f && std::isfinite(m.refraction_ratio))) {
            why = "RVCP_MATERIALS_SCATTER: material " + std::to_string(i) +
                  " (Dielectric) needs a finite refraction_ratio > 0";
            return false;
        }
    }
    return true;
}

static int upload_one(rvcp_ctx_t *ctx, const rvcp_material_t *materials, uint32_t n_materials,
                      const rvcp_vertex_t *vertices, uint32_t n_vertices,
                      const rvcp_face_t *faces, uint32_t n_faces,
                      const rvcp_sphere_t *spheres, uint32_t n_spheres,
                      const uint32_t *lum_face_ids, uint32_t n_lum_face_ids,
                      const uint32_t *lum_sphere_ids, uint32_t n_lum_sphere_ids)
{
    (void)lum_sphere_ids; (void)n_lum_sphere_ids;
    if (!ctx) return RVCP_E_INVALID;
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    SceneInput in;
    in.materials = materials; in.n_materials = n_materials;
    in.vertices = vertices; in.n_vertices = n_vertices;
    in.faces = faces; in.n_faces = n_faces;
    in.spheres = spheres; in.n_spheres = n_spheres;
    in.lum_face_ids = lum_face_ids; in.n_lum_face_ids = n_lum_face_ids;
    SceneTables tab;
    std::string err;
    if (prepare_scene(in, ctx->cfg.lum_id_std140_quirk != 0, tab, err) != RVCP_OK)
        return fail(ctx, RVCP_E_INVALID, err);
    if (ctx->materials == RVCP_MATERIALS_SCATTER &&
        !scatter_materials_ok(materials, n_materials, err))
        return fail(ctx, RVCP_E_INVALID, err);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<TriRecord> &tri = tab.tri;
    const float total = tab.light_total;

    free_scene(ctx);
    int rc;
    if ((rc = dev_upload<TriRecord>(ctx, &ctx->d_tri, tri.data(), n_faces)) ||
        (rc = dev_upload<rvcp_face_t>(ctx, &ctx->d_faces, faces, n_faces)) ||
        (rc = dev_upload<rvcp_vertex_t>(ctx, &ctx->d_verts, vertices, n_vertices)) ||
        (rc = dev_upload<MatRecord>(ctx, &ctx->d_mats, tab.mats.data(), n_materials)) ||
        (rc = dev_upload<FaceShade>(ctx, &ctx->d_shade, tab.shade.data(), n_faces)) ||
        (rc = dev_upload<LightRecord>(ctx, &ctx->d_lights, tab.lights.data(), n_lum_face_ids)) ||
        (rc = dev_upload<rvcp_material_t>(ctx, &ctx->d_rawmats, materials, n_materials)) ||
        (rc = dev_upload<rvcp_sphere_t>(ctx, &ctx->d_spheres, spheres, n_spheres)))
        return rc;
    {   // the albedo table of §4.12: the three floats as uploaded, 16 B per material
        std::vector<float> alb((size_t)n_materials * 4, 0.0f);
        for (uint32_t i = 0; i < n_materials; i++)
            std::memcpy(&alb[(size_t)i * 4], materials[i].albedo, 12);
        float4 *d_alb = nullptr;
        if ((rc = dev_upload<float4>(ctx, &d_alb, alb.data(), n_materials))) return rc;
        ctx->d_albedo = (float *)d_alb;
    }
    ctx->n_spheres = n_spheres;
    ctx->bvh_prefix = 0;
    std::shared_ptr<JitKernels> bvh_jit;
    if (ctx->cfg.accel == RVCP_ACCEL_BVH && n_faces > 0) {
        std::vector<float> pos((size_t)n_faces * 9);
        for (uint32_t i = 0; i < n_faces; i++)
            for (int v = 0; v < 3; v++)
                std::memcpy(&pos[(size_t)i * 9 + 3 * v], vertices[faces[i].vertices[v]].position, 12);
        const auto *P = reinterpret_cast<const float (*)[3][3]>(pos.data());
        // The hybrid: when the scene starts with a run of big faces (C5: the
        // Cornell room before 100 000 small triangles), those are tested by the specialised scan
        // -- at full lane utilisation, no dependent loads -- and the BVH holds only the rest, so
        // its boxes are tight and every ray enters it with the room's nearest hit as its bound.
        // Only with a specialised module for them (games101, specialize AUTO, the JIT's range);
        // the kernels without one test the prefix with the generic test.
        uint32_t K = 0;
        if (ctx->cfg.specialize == RVCP_SPECIALIZE_AUTO && ctx->cfg.integrator != RVCP_INTEGRATOR_LEGACY &&
            !RVCP_KNOB("RVCP_NO_BVH_PREFIX")) {
            K = bvh_big_prefix(P, n_faces, kJitMaxFaces);
            if (K < 8 || n_faces - K < 64 || !jit_scene_in_range(tri.data(), K)) K = 0;
            if (K) {
                std::string jerr;
                JitSpec spec;
                spec.bvh = true;
                spec.sampling = ctx->sampling;
                bvh_jit = jit_path_kernels(ctx->device, tri.data(), K, spec, jerr);
                HIP_TRY(ctx, hipSetDevice(ctx->device));
                if (!bvh_jit || !bvh_jit->bvh_path || !bvh_jit->bvh_primary) {
                    K = 0;
                    bvh_jit.reset();
                }
            }
        }
        std::vector<BvhNode> nodes;
        std::vector<uint32_t> order;
        int32_t root = 0;
        const int depth = bvh_build(P + K, n_faces - K, nodes, order, root);
        for (uint32_t &id : order)                       // the BVH's ids are faces K ...
            if (id != kBvhPadId) id += K;
        ctx->bvh_prefix = K;
        if (depth >= kBvhStack) return fail(ctx, RVCP_E_UNSUPPORTED, "BVH deeper than the traversal stack");
        // the leaf-ordered triangles packed as 10 floats per slot (v0, e1, e2, face id bits),
        // what the traversal reads (bvh_leaf); leaves start at even slots, so 16-B aligned.
        // A leaf reference is ~((start << 5) | (count - 1)) in an int32: start < 2^26.
        const size_t S = order.size();
        if (S >= (size_t(1) << 26))
            return fail(ctx, RVCP_E_UNSUPPORTED, "BVH leaf slots exceed 2^26 (mesh too large for the leaf encoding)");
        std::vector<TriRecord> btri((10 * S * 4 + sizeof(TriRecord) - 1) / sizeof(TriRecord) + 1);
        float *packed = reinterpret_cast<float *>(btri.data());
        for (size_t j = 0; j < S; j++) {
            if (order[j] == kBvhPadId) continue;        // padding slot: never referenced
            std::memcpy(packed + 10 * j, &tri[order[j]], 9 * sizeof(float));
            std::memcpy(packed + 10 * j + 9, &order[j], 4);
        }
        ctx->bvh_slots = 0;     // the packed records start the buffer
        std::vector<Bvh4Node> nodes4;
        int32_t root4 = 0;
        if (bvh4_collapse(nodes, root, nodes4, root4) > kBvhStack)
            return fail(ctx, RVCP_E_UNSUPPORTED, "BVH traversal stack bound exceeded");
        // only the byte-quantised copy (Bvh4QNode, 64 B) is traversed: it is uploaded alone,
        // at the start of the node buffer (FrameArgs::bvh_n4 = 0)
        std::vector<Bvh4QNode> q4;
        bvh4_quantize(nodes4, q4);
        std::vector<Bvh4Node> qbuf((q4.size() * sizeof(Bvh4QNode) + sizeof(Bvh4Node) - 1) / sizeof(Bvh4Node));
        if (!q4.empty()) std::memcpy(static_cast<void *>(qbuf.data()), q4.data(), q4.size() * sizeof(Bvh4QNode));
        ctx->bvh_n4 = 0;
        if ((rc = dev_upload<Bvh4Node>(ctx, &ctx->d_bvh_nodes, qbuf.data(), qbuf.size())) ||
            (rc = dev_upload<TriRecord>(ctx, &ctx->d_bvh_tris, btri.data(), btri.size())))
            return rc;
        ctx->bvh_root = root4;
        ctx->bvh_depth = depth;
    }
    // scene-specialised scan: compiled here, once per scene and process
    // Both slots are reset by an upload: the default one is filled here, the map one by the
    // first map render of this scene (jit_sampling[1] = -1).
    ctx->jit[0].reset();
    ctx->jit[1].reset();
    ctx->jit_err.clear();
    ctx->jit_tri.clear();
    ctx->jit_bvh = false;
    ctx->jit_lum = 0;
    ctx->jit_sampling[0] = ctx->sampling;
    ctx->jit_sampling[1] = -1;
    if (bvh_jit) {                            // the BVH hybrid's module (above)
        ctx->jit[0] = bvh_jit;
        ctx->jit_tri.assign(tri.begin(), tri.begin() + ctx->bvh_prefix);
        ctx->jit_bvh = true;
    }
    if (ctx->cfg.specialize == RVCP_SPECIALIZE_AUTO && ctx->cfg.accel == RVCP_ACCEL_NONE &&
        n_faces >= 1 && n_faces <= kJitMaxFaces && jit_scene_in_range(tri.data(), n_faces) &&
        !RVCP_KNOB("RVCP_NO_SPECIALIZE")) {
        const bool legacy = ctx->cfg.integrator == RVCP_INTEGRATOR_LEGACY;
        JitSpec spec;
        spec.legacy = legacy;
        spec.sphereless = n_spheres == 0;
        spec.lds_fits = n_spheres <= 64 && n_materials <= 64;
        spec.sampling = ctx->sampling;
        spec.spheres = spheres;
        spec.n_spheres = n_spheres;
        spec.n_materials = n_materials;
        for (uint32_t i = 0; i < n_lum_face_ids; i++)
            if (tab.lights[i].face < 64u) spec.lum_mask |= 1ull << tab.lights[i].face;
        ctx->jit_lum = spec.lum_mask;
        ctx->jit[0] = jit_path_kernels(ctx->device, tri.data(), n_faces, spec, ctx->jit_err);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (!legacy) ctx->jit_tri = tri;      // (mode 2 has one sampling: nothing to ask again)
    }
    ctx->rcp_fast = scan_rcp_fast_scene(tri.data(), n_faces);
    ctx->n_faces = n_faces;
    ctx->n_verts = n_vertices;
    ctx->n_mats = n_materials;
    ctx->has_metal = false;
    for (uint32_t i = 0; i < n_materials; i++)
        if (materials[i].ty == 1u) ctx->has_metal = true;
    ctx->n_lights = n_lum_face_ids;
    ctx->lights_same = n_lum_face_ids >= 1;
    for (uint32_t i = 1; i < n_lum_face_ids; i++)
        if (tab.lights[i].face != tab.lights[0].face) ctx->lights_same = false;
    ctx->light_total = total;
    ctx->light_pdf = 1.0f / total;
    ctx->h_rawmats.assign(materials, materials + n_materials);
    ctx->has_scene = true;
    return RVCP_OK;
}

static int impl_upload_scene_file(rvcp_ctx_t *ctx, const char *path, rvcp_camera_t *out_camera)
{
    if (!ctx) return RVCP_E_INVALID;
    SceneFile sf;
    std::string err;
    if (read_scene_file(path, sf, err) != RVCP_OK) return fail(ctx, RVCP_E_INVALID, err);
    const rvcp_lengths_t &L = sf.lengths;
    const int rc = rvcp_upload_scene(ctx, sf.materials.data(), L.materials_len, sf.vertices.data(),
                                     L.vertices_len, sf.faces.data(), L.faces_len, sf.spheres.data(),
                                     L.spheres_len, sf.lum_face_ids.data(), L.luminous_face_id_len,
                                     sf.lum_sphere_ids.data(), L.luminous_sphere_id_len);
    if (rc == RVCP_OK && out_camera) *out_camera = sf.camera;
    return rc;
}

uint32_t rvcp_shard_rows(uint32_t height, uint32_t shard_index, uint32_t shard_count)
{
    if (shard_count == 0 || shard_index >= shard_count) return 0;
    const uint32_t stripes = (height + 7) / 8;
    uint32_t rows = 0;
    for (uint32_t s = shard_index; s < stripes; s += shard_count)
        rows += (s + 1) * 8 <= height ? 8 : height - s * 8;
    return rows;
}

// The scene's specialised module for a default or a map render with the context's bounce
// sampling, asked for again with what upload asked (jit_tri, jit_bvh) by the first such render
// after rvcp_set_sampling changed the mode -- for a map render also by the first of the scene:
// from the process's module cache, the disk cache, or hipRTC.  Without one (no module for this
// scene, or the compilation failed) the generic kernels of that build run; a module of the other
// mode is never kept.  The default slot's error goes to jit_err; the map slot's is dropped.
static void jit_for_render(rvcp_ctx_t *ctx, bool map)
{
    ctx->jit_sampling[map] = ctx->sampling;
    if (ctx->jit_tri.empty()) return;
    std::shared_ptr<JitKernels> &jit = ctx->jit[map];
    jit.reset();
    std::string map_err;
    if (!map) ctx->jit_err.clear();
    JitSpec spec;
    spec.bvh = ctx->jit_bvh;
    spec.sampling = ctx->sampling;
    spec.spp_map = map;
    spec.lum_mask = ctx->jit_lum;
    jit = jit_path_kernels(ctx->device, ctx->jit_tri.data(), (uint32_t)ctx->jit_tri.size(), spec,
                           map ? map_err : ctx->jit_err);
    (void)hipSetDevice(ctx->device);
    if (ctx->jit_bvh && jit && (!jit->bvh_path || !jit->bvh_primary)) jit.reset();
}

// What plan_frame (rvcp_frame_plan.cpp) decides a render from: the config, the scene, the device's
// capacities for the context's bounce sampling, the scene's specialised module and the frames.
// A map render (spp_hint > 0): the hint in place of cfg.spp, the map kernels' capacities and the
// map module.
static FramePlanIn frame_plan_input(const rvcp_ctx_t *ctx, uint32_t n_frames, uint32_t frame_px,
                                    uint32_t stride, uint32_t spp_hint = 0)
{
    const bool cosine = ctx->sampling == RVCP_SAMPLING_COSINE;
    const bool map = spp_hint > 0;
    FramePlanIn in;
    in.integrator = ctx->cfg.integrator;
    in.kernel_variant = ctx->cfg.kernel_variant;
    in.accel = ctx->cfg.accel;
    in.spp = map ? spp_hint : ctx->cfg.spp;
    in.max_bounces = ctx->cfg.max_bounces;
    in.attenuation_stop_eps = ctx->cfg.attenuation_stop_eps;
    in.ray_t_min = ctx->cfg.ray_t_min;
    in.grid_waves_per_simd = ctx->cfg.grid_waves_per_simd;
    in.n_faces = ctx->n_faces;
    in.bvh_prefix = ctx->bvh_prefix;
    in.n_simds = ctx->n_simds;
    const rvcp_ctx::Capacity &cap = ctx->capacity[cosine][map];
    std::memcpy(in.grid_capacity, cap.grid, sizeof(in.grid_capacity));
    in.bvh_capacity = cap.bvh;
    in.legacy_capacity = ctx->legacy_capacity;
    if (const JitKernels *jk = ctx->jit[map].get()) {
        in.module = true;
        in.blocks_per_cu5 = jk->blocks_per_cu5;
        in.blocks_per_cu6 = jk->blocks_per_cu6;
        in.blocks_per_cu_bvh = jk->blocks_per_cu_bvh;
        in.blocks_per_cu_legacy = jk->blocks_per_cu_legacy;
        in.has_legacy = jk->legacy != nullptr;
        in.has_bvh_path = jk->bvh_path != nullptr;
        in.has_bvh_primary = jk->bvh_primary != nullptr;
    }
    in.n_frames = n_frames;
    in.frame_px = frame_px;
    in.stride = stride;
    if (const char *c = RVCP_KNOB("RVCP_DEBUG_SPREAD")) in.spread_min = (uint32_t)std::atoi(c);
    return in;
}

// The shading parameters of a games101 launch: the configuration's, the scene's light table and
// the constants derived from them (the render's and the path queries' FrameArgs share them)
static void shading_frame_args(const rvcp_ctx_t *ctx, FrameArgs &A)
{
    A.max_bounces = ctx->cfg.max_bounces;
    A.att_stop = ctx->cfg.attenuation_stop_eps;
    A.t_min = ctx->cfg.ray_t_min;
    A.t_max = ctx->cfg.ray_t_max;
    A.rr = ctx->cfg.rr_probability;
    A.eps = ctx->cfg.eps;
    A.n_lights = ctx->n_lights;
    A.lights_same = ctx->lights_same ? 1u : 0u;
    A.rcp_fast = ctx->rcp_fast ? 1u : 0u;
    A.has_metal = ctx->has_metal ? 1u : 0u;
    A.light_total = ctx->light_total;
    A.light_pdf = ctx->light_pdf;
    {   // :465-471: denom = max(0.1, pdf) * rr, pdf = 0.5 / 3.1415926 (cos > 0) or 0; IEEE 1/denom
        const float pdf1 = 0.5f / 3.1415926f;
        A.brdf_den[1] = std::fmax(0.1f, pdf1) * A.rr;
        A.brdf_den[0] = std::fmax(0.1f, 0.0f) * A.rr;
        A.brdf_rcp[1] = 1.0f / A.brdf_den[1];
        A.brdf_rcp[0] = 1.0f / A.brdf_den[0];
    }
    A.cos_k = 3.1415926f / A.rr;        // the cosine-weighted bounce's factor k = PI_F / rr
}

// kernel_variant of a frame rendered with material scattering (rvcp.h)
constexpr int32_t kScatterStatsCode = 11;

// One whole frame with material scattering (rvcp_set_materials), the composition
// §4.20 proves equal to a frame: the frame's primary rays and seeds into buffers of the context,
// path_scatter_kernel over them into the linear frame, the tone map into RGBA8.  render_frames
// has checked the arguments; the statistics are the render's (d_counters, ev0 / evm / ev1).
static int render_scatter(rvcp_ctx_t *ctx, const rvcp_push_constant_t &push, uint32_t width,
                          uint32_t height, void *d_rgba8, void *d_linear_rgb, hipStream_t s)
{
    const uint32_t n = width * height;
    int rc;
    if ((rc = grow(ctx, &ctx->d_ms_rays, &ctx->cap_ms_rays, n, sizeof(rvcp_ray_t))) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_ms_seeds, &ctx->cap_ms_seeds, n, sizeof(float))) != RVCP_OK) return rc;
    float *lin = (float *)d_linear_rgb;
    if (!lin) {
        if ((rc = grow(ctx, (void **)&ctx->d_acc, &ctx->cap_acc, n, 12)) != RVCP_OK) return rc;
        lin = ctx->d_acc;
    }
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    primary_frame_args(ctx, push, width, height, A);
    A.shard_index = 0;
    A.shard_count = 1;
    A.n_pixels = n;
    A.spp = ctx->cfg.spp;
    shading_frame_args(ctx, A);
    A.n_mats = ctx->n_mats;
    A.n_simds = ctx->n_simds;
    ctx->last_timeline_waves = 0;
    // a gather of this context's previous frame may still read the caller's buffer
    if (ctx->gather_on_gstream) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evg1, 0));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, kCounterWords * sizeof(unsigned long long), s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, s));
    int launch_rc = rvcp_launch_primary_rays(&A, 0, n, ctx->d_ms_rays, s);
    if (launch_rc == 0) launch_rc = rvcp_launch_primary_seeds(&A, n, ctx->d_ms_seeds, s);
    HIP_TRY(ctx, hipEventRecord(ctx->evm, s));
    if (launch_rc == 0)
        launch_rc = rvcp_launch_path_scatter(&A, ctx->d_tri, ctx->d_shade, ctx->d_mats,
                                             ctx->d_rawmats, ctx->d_lights, ctx->d_bvh_nodes,
                                             ctx->d_bvh_tris, ctx->d_ms_rays, ctx->d_ms_seeds, lin,
                                             ctx->d_counters, ctx->cfg.grid_waves_per_simd, s);
    if (launch_rc == 0)
        launch_rc = rvcp_launch_tonemap(lin, n, ctx->d_gamma, (uint32_t *)d_rgba8, s);
    if (launch_rc != 0) return fail(ctx, RVCP_E_HIP, std::string("kernel launch failed: ") +
                                                         hipGetErrorString(hipGetLastError()));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    ctx->pending = true;
    ctx->render_stream = s;
    ctx->last_trivial = false;
    ctx->last_scatter = true;
    ctx->last_variant = kScatterStatsCode;
    ctx->last_pixels = n;
    ctx->last_spp = A.spp;
    ctx->last_map = false;
    ctx->last_shard_index = 0;
    ctx->last_shard_count = 1;
    ctx->last_width = width;
    ctx->last_height = height;
    return RVCP_OK;
}

// n_frames consecutive frames of one shard (pushes[k] for frame k) into outputs laid out frame
// after frame, `slot` = the largest shard's rows apart (rvcp_render_frames_async); n_frames = 1
// is rvcp_render_shard_async.  d_spp_map (rvcp_render_spp_map_async; one whole frame): the
// frame's per-pixel sample counts, traced by the map builds of the pre-pass family, spp_hint in
// place of cfg.spp in the plan.
static int render_frames(rvcp_ctx_t *ctx, const rvcp_push_constant_t *pushes, uint32_t n_frames,
                         uint32_t width, uint32_t height, uint32_t shard_index,
                         uint32_t shard_count, void *d_rgba8, void *d_linear_rgb, void *stream,
                         const uint32_t *d_spp_map = nullptr, uint32_t spp_hint = 0)
{
    if (!ctx) return RVCP_E_INVALID;
    const bool map = d_spp_map != nullptr;
    const rvcp_push_constant_t *push = pushes;
    if (!push || n_frames == 0 || !d_rgba8 || width == 0 || height == 0 || shard_count == 0 ||
        shard_index >= shard_count)
        return fail(ctx, RVCP_E_INVALID, "invalid render arguments");
    if ((uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "frame too large (W*H must be < 2^31)");
    // frame k of a batch starts `stride` pixels after frame k-1 (the largest shard's pixels)
    const uint32_t stride = rvcp_shard_rows(height, 0, shard_count) * width;
    if ((uint64_t)n_frames * stride >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "batch too large (n_frames x shard pixels must be < 2^31)");
    if (n_frames > 1 && !ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "frame batches drive one GPU (n_gpus = 1)");
    if (!ctx->has_scene) return fail(ctx, RVCP_E_NO_SCENE, "render before rvcp_upload_scene");
    for (uint32_t k = 0; k < n_frames; k++)
        if (!primary_t_range_ok(pushes[k], width, height))
            return fail(ctx, RVCP_E_INVALID, "camera t_far x t_coef must stay below 2^24 (the "
                        "shader's miss test t_max + 1, :287, :424)");
    // one frame in flight per context: its surface list, counters and events are the frame's
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    // material scattering (rvcp_set_materials) renders one whole frame
    if (ctx->materials == RVCP_MATERIALS_SCATTER) {
        if (map)
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER renders no per-pixel "
                        "sample count (rvcp_render_spp_map_async, the adaptive switch)");
        if (n_frames > 1)
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER renders no frame batch "
                        "(n_frames must be 1)");
        if (shard_count > 1)
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER renders whole frames "
                        "(shard_count must be 1)");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (ctx->materials == RVCP_MATERIALS_SCATTER)
        return render_scatter(ctx, *push, width, height, d_rgba8, d_linear_rgb, s);

    // the cosine-weighted bounce (rvcp_set_sampling): its kernels, and a
    // specialised module compiled for it
    const bool cosine = ctx->sampling == RVCP_SAMPLING_COSINE;
    if (ctx->jit_sampling[map] != ctx->sampling) jit_for_render(ctx, map);

    // the plan: schedule, specialised kernels and grid (rvcp_frame_plan.cpp)
    const uint32_t frame_px = rvcp_shard_rows(height, shard_index, shard_count) * width;
    const uint32_t split_px = frame_px * n_frames;          // the queue of the whole batch
    const JitKernels *jk = ctx->jit[map].get();
    const FramePlanIn in = frame_plan_input(ctx, n_frames, frame_px, stride, map ? spp_hint : 0u);
    const FramePlan P = plan_frame(in);
    if (map && P.status == RVCP_OK && !P.trivial && !P.legacy && P.variant < 3)
        return fail(ctx, RVCP_E_UNSUPPORTED, "a per-pixel sample count needs a pre-pass schedule "
                    "(schedules 3-6, 10, or the BVH path kernel)");
    if (P.status != RVCP_OK)
        return fail(ctx, P.status, "frame batches need a pre-pass schedule of the games101 "
                    "integrator (schedules 3-6, 10, or the BVH path kernel) or mode 2");
    const bool launches = !P.trivial && frame_px > 0;           // a path kernel runs
    const bool lin_staged = P.legacy || P.variant >= 3;         // ... that leaves linear colours

    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    primary_frame_args(ctx, *push, width, height, A);
    A.shard_index = shard_index;
    A.shard_count = shard_count;
    A.n_pixels = frame_px;
    A.spp = map ? spp_hint : ctx->cfg.spp;      // (a map build's kernels do not read it)
    shading_frame_args(ctx, A);
    A.want_linear = d_linear_rgb ? 1u : 0u;
    A.variant = P.variant;
    A.n_spheres = P.legacy ? ctx->n_spheres : 0u;
    A.n_mats = ctx->n_mats;
    A.n_simds = ctx->n_simds;
    A.static_chunk = P.static_chunk;
    A.static_chunks = P.static_chunks;
    A.dyn_chunk = kDynChunk;
    A.chunk_min = kMinChunk;
    A.chunk_window = kChunkWindow;
    if (const char *c = RVCP_KNOB("RVCP_DEBUG_CHUNK")) {   // fixed grab (experiments)
        const int v = std::atoi(c);
        if (v >= 1 && v <= (int)kDynChunk) A.dyn_chunk = A.chunk_min = (uint32_t)v;   // <= 64: mode 2 prefills a grab into 64 LDS slots
    }
    if (const char *c = RVCP_KNOB("RVCP_DEBUG_CHUNK_WINDOW")) {
        const int v = std::atoi(c);
        if (v >= 1) A.chunk_window = (uint32_t)v;
    }
    A.spread_min = in.spread_min;
    if (const char *c = RVCP_KNOB("RVCP_DEBUG_EARLY_TAIL")) A.early_tail = (uint32_t)std::atoi(c);
    if (P.cams && P.legacy) {
        // mode 2 has no pre-pass: its one kernel queues the batch's pixels frame after frame
        // and reads each frame's camera and time from d_cams (FrameArgs::batch_cams)
        A.frame_pixels = frame_px;
        A.frame_stride = stride;
        A.n_pixels = split_px;
    }

    // the buffers the launch needs.  A batch's cameras and times in device memory: mode 2's one
    // kernel and the pre-pass schedules' one pre-pass launch read them per frame
    int rc;
    if (P.cams) {
        if ((rc = grow_cams(ctx, n_frames)) != RVCP_OK) return rc;
        if (P.legacy) A.batch_cams = ctx->d_cams;
    }
    ctx->last_timeline_waves = 0;
    if (launches && lin_staged && RVCP_KNOB("RVCP_DEBUG_TIMELINE")) {
        const size_t waves = (size_t)P.blocks * P.wpb;
        if ((rc = grow(ctx, (void **)&ctx->d_timeline, &ctx->cap_timeline, waves, 64)) != RVCP_OK)
            return rc;
        A.timeline = ctx->d_timeline;
        ctx->last_timeline_waves = waves;
    }
    // the mode-2 and v3-family kernels leave linear colours and tonemap_kernel stores
    // the bytes: into the caller's linear buffer, else the context's scratch
    float *lin = (float *)d_linear_rgb;
    if (launches && lin_staged && !lin) {
        if ((rc = grow(ctx, (void **)&ctx->d_acc, &ctx->cap_acc, P.out_px, 12)) != RVCP_OK) return rc;
        lin = ctx->d_acc;
    }
    // the surface list of the pre-pass schedules, shared by the batch
    if (launches && !P.legacy && P.variant >= 3 &&
        (rc = grow(ctx, (void **)&ctx->d_surf, &ctx->cap_surf, split_px, sizeof(SurfRecord))) != RVCP_OK)
        return rc;

    // per frame of the batch: camera, time, pixel base
    std::vector<FrameArgs> FA(n_frames, A);
    for (uint32_t k = 1; k < n_frames; ++k) {
        camera_constants(pushes[k], width, height, FA[k]);
        FA[k].pix_base = k * stride;
    }
    if (P.cams) {
        for (uint32_t k = 0; k < n_frames; ++k) pack_frame_cam(FA[k], ctx->h_cams + 16 * (size_t)k);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cams, ctx->h_cams, (size_t)n_frames * 64,
                                    hipMemcpyHostToDevice, s));
    }

    // a gather of this context's previous frame may still read the caller's shard buffer
    if (ctx->gather_on_gstream) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evg1, 0));
    // ... and a plan step of this context may still write the map
    if (map && ctx->stage[ST_PLAN].recorded)
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->stage[ST_PLAN].ev1, 0));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, kCounterWords * sizeof(unsigned long long), s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, s));
    int launch_rc = 0;
    if (frame_px == 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->evm, s));
    } else if (P.trivial) {
        HIP_TRY(ctx, hipEventRecord(ctx->evm, s));
        launch_rc = rvcp_launch_fill((uint32_t *)d_rgba8, (float *)d_linear_rgb, P.out_px,
                                     0xFF000000u, s);
    } else if (P.legacy) {
        HIP_TRY(ctx, hipEventRecord(ctx->evm, s));
        launch_rc = rvcp_launch_legacy(&A, ctx->d_tri, ctx->d_shade, ctx->d_spheres, ctx->d_rawmats,
                                       ctx->d_unorm, (uint32_t *)d_rgba8, lin, ctx->d_counters,
                                       P.blocks, s, P.spec_legacy ? (void *)jk->legacy : nullptr);
    } else {
        // the games101 kernels of the context's build (kKernelBuilds; a map render has
        // P.variant >= 3: checked above)
        const KernelBuild &build = *kKernelBuilds[cosine][map];
        PathLaunch L{};
        L.args = FA.data();
        L.n_frames = n_frames;
        L.frame_stride = stride;
        L.tri = ctx->d_tri;
        L.faces = ctx->d_faces;
        L.verts = ctx->d_verts;
        L.mats = ctx->d_mats;
        L.lights = ctx->d_lights;
        L.gamma_t = ctx->d_gamma;
        L.out_rgba = (uint32_t *)d_rgba8;
        L.out_lin = lin;
        L.counters = ctx->d_counters;
        L.surf = ctx->d_surf;
        L.shade = ctx->d_shade;
        L.bvh_nodes = ctx->d_bvh_nodes;
        L.bvh_tris = ctx->d_bvh_tris;
        L.grid_blocks = P.blocks;
        L.stream = s;
        L.main_event = ctx->evm;
        L.spec_path_fn = P.spec ? (void *)(P.variant == 6 ? jk->path6 : jk->path5)
                                : P.spec_bvh ? (void *)jk->bvh_path : nullptr;
        L.spec_pre_fn = P.spec && jit_spec_prepass() ? (void *)jk->primary
                                                     : P.spec_bvh ? (void *)jk->bvh_primary : nullptr;
        L.cams = P.prepass_batched ? ctx->d_cams : nullptr;
        L.spp_map = d_spp_map;
        if (P.variant >= 3) {
            // (the launcher records evm itself, between the pre-pass and the path kernel)
            launch_rc = build.launch_prepass(L);
        } else {
            HIP_TRY(ctx, hipEventRecord(ctx->evm, s));
            launch_rc = build.launch(L);
        }
    }
    if (launch_rc != 0) return fail(ctx, RVCP_E_HIP, std::string("kernel launch failed: ") +
                                                         hipGetErrorString(hipGetLastError()));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    ctx->pending = true;
    ctx->render_stream = s;
    ctx->last_trivial = P.trivial;
    ctx->last_scatter = false;
    ctx->last_variant = P.stats_code;
    ctx->last_pixels = (uint64_t)frame_px * n_frames;       // stats cover the whole batch
    ctx->last_spp = A.spp;
    ctx->last_map = map;
    ctx->last_shard_index = shard_index;
    ctx->last_shard_count = shard_count;
    ctx->last_width = width;
    ctx->last_height = height;
    return RVCP_OK;
}

static int impl_render_shard_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                                   uint32_t height, uint32_t shard_index, uint32_t shard_count,
                                   void *d_rgba8, void *d_linear_rgb, void *stream)
{
    return render_frames(ctx, push, 1, width, height, shard_index, shard_count, d_rgba8,
                         d_linear_rgb, stream);
}

static int impl_render_frames_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *pushes,
                                    uint32_t n_frames, uint32_t width, uint32_t height,
                                    uint32_t shard_index, uint32_t shard_count, void *d_rgba8,
                                    void *d_linear_rgb, void *stream)
{
    return render_frames(ctx, pushes, n_frames, width, height, shard_index, shard_count, d_rgba8,
                         d_linear_rgb, stream);
}

static int impl_render_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                      uint32_t height, void *d_rgba8, void *d_linear_rgb, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "rvcp_render_async drives one GPU; use rvcp_render for n_gpus > 1");
    return rvcp_render_shard_async(ctx, push, width, height, 0, 1, d_rgba8, d_linear_rgb, stream);
}

// rvcp_render_async with a per-pixel sample count; every rejection comes before
// any launch
static int impl_render_spp_map_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                                     uint32_t width, uint32_t height, const void *d_spp_map,
                                     uint32_t spp_hint, void *d_rgba8, void *d_linear_rgb,
                                     void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !d_spp_map || !d_rgba8 || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid map render arguments");
    if (spp_hint < 1 || spp_hint > RVCP_SPP_MAP_MAX)
        return fail(ctx, RVCP_E_INVALID, "spp_hint must be in 1..256");
    if ((uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "frame too large (W*H must be < 2^31)");
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, "a per-pixel sample count is implemented for the "
                    "games101 integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "rvcp_render_spp_map_async drives one GPU (n_gpus = 1)");
    return render_frames(ctx, push, 1, width, height, 0, 1, d_rgba8, d_linear_rgb, stream,
                         (const uint32_t *)d_spp_map, spp_hint);
}

static int impl_wait(rvcp_ctx_t *ctx, rvcp_stats_t *stats)
{
    return rvcp_sync_stats(ctx, stats);
}

static int impl_sync_stats(rvcp_ctx_t *ctx, rvcp_stats_t *stats)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->pending) return fail(ctx, RVCP_E_INVALID, "no render in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        unsigned long long c[kCounterWords] = {};
        HIP_TRY(ctx, hipMemcpy(c, ctx->d_counters, sizeof(c), hipMemcpyDeviceToHost));
        // the path kernel's per-wave clock stamps (clock_stamp): shader-clock ticks over
        // 100-MHz ticks, summed over its waves
        stats->shader_clock_ghz = c[kClockWord + 1]
            ? 0.1 * (double)c[kClockWord] / (double)c[kClockWord + 1] : 0.0;
        stats->kernel_ms = ms;
        float ms_main = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms_main, ctx->evm, ctx->ev1));
        stats->main_kernel_ms = ms_main;
        stats->traversals_executed = c[0];
        // the reference re-traces the (RNG-independent) primary ray in every sample
        stats->traversals = ctx->last_trivial ? 0 : c[0] + ctx->last_pixels * (ctx->last_spp - 1);
        if (ctx->last_scatter) {
            // its kernel counts as the shader does, the kept first hit once per sample (no
            // traversal at all in a frame whose configuration ends every sample at once)
            const uint64_t reused = ctx->last_pixels * (ctx->last_spp - 1);
            stats->traversals = c[0];
            stats->traversals_executed = c[0] >= reused ? c[0] - reused : 0;
        }
        stats->samples = ctx->last_pixels * ctx->last_spp;
        if (ctx->last_map) {
            // a map render: the pre-pass's sum of the clamped counts (0 for a trivial frame, whose
            // fill reads no map)
            const uint64_t sum = c[kSppSumWord];
            stats->samples = sum;
            stats->traversals = ctx->last_trivial ? 0 : c[0] + (sum - ctx->last_pixels);
        }
        stats->faces = ctx->n_faces;
        stats->kernel_variant = ctx->last_variant;
        stats->wave_iterations = c[2];
    }
    if (ctx->last_timeline_waves) {
        std::vector<unsigned long long> t(8 * ctx->last_timeline_waves);
        HIP_TRY(ctx, hipMemcpy(t.data(), ctx->d_timeline, t.size() * 8, hipMemcpyDeviceToHost));
        const char *path = RVCP_KNOB("RVCP_DEBUG_TIMELINE");
        if (FILE *f = path ? std::fopen(path, "ab") : nullptr) {
            std::fwrite(t.data(), 8, t.size(), f);
            std::fclose(f);
        }
        ctx->last_timeline_waves = 0;
    }
    ctx->pending = false;           // a render is waited for once
    return RVCP_OK;
}

// n_gpus > 1: every GPU renders its stripes packed (shard k of N on GPU k), then each shard
// is copied into the frame on ctx->device with one strided copy (stripe j of shard k ->
// frame rows 8(jN + k) .. +8), over xGMI when the GPUs differ.  Stats are summed over shards;
// kernel_ms is the slowest shard's.
static int render_multi(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t W,
                        uint32_t H, bool want_lin, rvcp_stats_t *stats)
{
    const uint32_t N = (uint32_t)ctx->subs.size() + 1;
    int rc;
    // 1. launch every shard (shard 0 renders on ctx itself, into a packed buffer of its own)
    for (uint32_t k = 1; k < N; k++) {
        const size_t px = (size_t)rvcp_shard_rows(H, k, N) * W;
        if ((rc = grow_packed(ctx, ctx->subs[k - 1]->device, &ctx->shard_rgba[k - 1],
                              &ctx->shard_lin[k - 1], &ctx->shard_cap[k - 1], px, want_lin)) != RVCP_OK)
            return rc;
    }
    // shard 0 needs its own packed buffer too: reuse the staging's tail is not possible, so
    // keep it in shard_rgba[-1] semantics via a dedicated allocation on ctx
    const size_t px0 = (size_t)rvcp_shard_rows(H, 0, N) * W;
    if ((rc = grow_packed(ctx, ctx->device, &ctx->d_pack_rgba, &ctx->d_pack_lin, &ctx->cap_surf_pack,
                          px0, want_lin)) != RVCP_OK)
        return rc;
    for (uint32_t k = 0; k < N; k++) {
        rvcp_ctx *c = k == 0 ? ctx : ctx->subs[k - 1];
        uint32_t *d_rgba = k == 0 ? ctx->d_pack_rgba : ctx->shard_rgba[k - 1];
        float *d_lin = want_lin ? (k == 0 ? ctx->d_pack_lin : ctx->shard_lin[k - 1]) : nullptr;
        if ((rc = rvcp_render_shard_async(c, push, W, H, k, N, d_rgba, d_lin, c->stream)) != RVCP_OK) {
            if (k > 0) ctx->err = "shard " + std::to_string(k) + ": " + c->err;
            (void)hipSetDevice(ctx->device);
            return rc;
        }
    }
    // 2. wait for each shard and copy its stripes into the frame on ctx->device
    rvcp_stats_t total;
    std::memset(&total, 0, sizeof(total));
    for (uint32_t k = 0; k < N; k++) {
        rvcp_ctx *c = k == 0 ? ctx : ctx->subs[k - 1];
        rvcp_stats_t st;
        if ((rc = rvcp_sync_stats(c, &st)) != RVCP_OK) {
            if (k > 0) ctx->err = "shard " + std::to_string(k) + ": " + c->err;
            (void)hipSetDevice(ctx->device);
            return rc;
        }
        total.kernel_ms = st.kernel_ms > total.kernel_ms ? st.kernel_ms : total.kernel_ms;
        total.main_kernel_ms = st.main_kernel_ms > total.main_kernel_ms ? st.main_kernel_ms : total.main_kernel_ms;
        total.traversals += st.traversals;
        total.traversals_executed += st.traversals_executed;
        total.samples += st.samples;
        total.wave_iterations += st.wave_iterations;
        total.faces = st.faces;
        total.kernel_variant = st.kernel_variant;
        if (k == 0) total.shader_clock_ghz = st.shader_clock_ghz;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const uint32_t stripes = (H + 7) / 8;
        const uint32_t full = H / 8;                       // stripes with 8 rows
        uint32_t n_full = 0;                               // full stripes of shard k
        for (uint32_t s = k; s < full; s += N) n_full++;
        const uint8_t *src = (const uint8_t *)(k == 0 ? ctx->d_pack_rgba : ctx->shard_rgba[k - 1]);
        const float *srcl = k == 0 ? ctx->d_pack_lin : ctx->shard_lin[k - 1];
        for (int pass = 0; pass < (want_lin ? 2 : 1); pass++) {
            const size_t bpp = pass == 0 ? 4 : 12;
            const uint8_t *sp = pass == 0 ? src : (const uint8_t *)srcl;
            uint8_t *dp = pass == 0 ? (uint8_t *)ctx->d_rgba : (uint8_t *)ctx->d_lin;
            if (n_full)
                HIP_TRY(ctx, hipMemcpy2DAsync(dp + (size_t)8 * k * W * bpp, (size_t)8 * N * W * bpp,
                                              sp, (size_t)8 * W * bpp, (size_t)8 * W * bpp, n_full,
                                              hipMemcpyDefault, ctx->stream));
            // a last, partial stripe (H % 8 rows), if it is shard k's
            if (full < stripes && (full % N) == k) {
                const size_t rows = H - 8 * full;
                HIP_TRY(ctx, hipMemcpyAsync(dp + (size_t)8 * full * W * bpp,
                                            sp + (size_t)8 * n_full * W * bpp, rows * W * bpp,
                                            hipMemcpyDefault, ctx->stream));
            }
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) *stats = total;
    return RVCP_OK;
}

static int impl_render(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                uint32_t height, uint8_t *out_rgba8, float *out_linear_rgb, rvcp_stats_t *stats)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!out_rgba8) return fail(ctx, RVCP_E_INVALID, "out_rgba8 is required");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "invalid frame size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)width * height;
    int rc;
    if ((rc = grow(ctx, (void **)&ctx->d_rgba, &ctx->cap_rgba, npx, 4)) != RVCP_OK) return rc;
    if (out_linear_rgb && (rc = grow(ctx, (void **)&ctx->d_lin, &ctx->cap_lin, npx, 12)) != RVCP_OK)
        return rc;
    if (ctx->subs.empty()) {
        rc = rvcp_render_shard_async(ctx, push, width, height, 0, 1, ctx->d_rgba,
                                     out_linear_rgb ? ctx->d_lin : nullptr, ctx->stream);
        if (rc != RVCP_OK) return rc;
        if ((rc = rvcp_sync_stats(ctx, stats)) != RVCP_OK) return rc;
    } else if ((rc = render_multi(ctx, push, width, height, out_linear_rgb != nullptr, stats)) != RVCP_OK) {
        return rc;
    }
    HIP_TRY(ctx, hipMemcpy(out_rgba8, ctx->d_rgba, npx * 4, hipMemcpyDeviceToHost));
    if (out_linear_rgb) HIP_TRY(ctx, hipMemcpy(out_linear_rgb, ctx->d_lin, npx * 12, hipMemcpyDeviceToHost));
    return RVCP_OK;
}

static int impl_mandelbrot(rvcp_ctx_t *ctx, const rvcp_mandelbrot_push_t *push, uint32_t width,
                    uint32_t height, uint8_t *out_rgba8, float *out_value, rvcp_stats_t *stats)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !out_rgba8 || width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "invalid mandelbrot arguments");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)width * height;
    int rc;
    if ((rc = grow(ctx, (void **)&ctx->d_rgba, &ctx->cap_rgba, npx, 4)) != RVCP_OK) return rc;
    // the float escape values reuse the linear-RGB staging buffer (npx floats <= 3 npx)
    if (out_value && (rc = grow(ctx, (void **)&ctx->d_lin, &ctx->cap_lin, npx, 12)) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (rvcp_launch_mandelbrot(push->position[0], push->position[1], push->scale, width, height,
                               ctx->d_unorm, ctx->d_rgba, out_value ? ctx->d_lin : nullptr,
                               ctx->stream) != 0)
        return fail(ctx, RVCP_E_HIP, "mandelbrot launch failed");
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        float ms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        stats->kernel_ms = ms;
        stats->main_kernel_ms = ms;
    }
    HIP_TRY(ctx, hipMemcpy(out_rgba8, ctx->d_rgba, npx * 4, hipMemcpyDeviceToHost));
    if (out_value) HIP_TRY(ctx, hipMemcpy(out_value, ctx->d_lin, npx * 4, hipMemcpyDeviceToHost));
    return RVCP_OK;
}

// ---- what the post-process steps share --------------------------------------------------

// Opens step `id` on stream s: its events exist, s waits for a render pending on this context
// (when it runs on another stream) and for the steps of kStageBehind[id], and the start event is
// recorded.  Each event is created if it is missing, so a creation that failed is tried again.
static int stage_begin(rvcp_ctx_t *ctx, StageId id, hipStream_t s)
{
    Stage &st = ctx->stage[id];
    if (!st.ev0) HIP_TRY(ctx, hipEventCreate(&st.ev0));
    if (!st.ev1) HIP_TRY(ctx, hipEventCreate(&st.ev1));
    if (ctx->pending && ctx->render_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev1, 0));
    for (int k = 0; k < N_STAGES; ++k)
        if ((kStageBehind[id] >> k & 1u) && ctx->stage[k].recorded)
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->stage[k].ev1, 0));
    HIP_TRY(ctx, hipEventRecord(st.ev0, s));
    return RVCP_OK;
}

static int stage_end(rvcp_ctx_t *ctx, StageId id, hipStream_t s)
{
    Stage &st = ctx->stage[id];
    HIP_TRY(ctx, hipEventRecord(st.ev1, s));
    st.recorded = true;
    st.pending = true;
    return RVCP_OK;
}

static int stage_sync(rvcp_ctx_t *ctx, StageId id, float *ms)
{
    Stage &st = ctx->stage[id];
    HIP_TRY(ctx, hipEventSynchronize(st.ev1));
    if (ms) HIP_TRY(ctx, hipEventElapsedTime(ms, st.ev0, st.ev1));
    st.pending = false;
    return RVCP_OK;
}

// rvcp_*_wait of one step; `none` is its "no ... in flight" text
static int stage_wait(rvcp_ctx_t *ctx, StageId id, const char *none, float *ms)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->stage[id].pending) return fail(ctx, RVCP_E_INVALID, none);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return stage_sync(ctx, id, ms);
}

// ... and of a pair of steps: whichever of the two are pending (0 ms for the other)
static int stage_wait2(rvcp_ctx_t *ctx, StageId a, StageId b, const char *none, float *a_ms,
                       float *b_ms)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->stage[a].pending && !ctx->stage[b].pending) return fail(ctx, RVCP_E_INVALID, none);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (a_ms) *a_ms = 0.0f;
    if (b_ms) *b_ms = 0.0f;
    int rc;
    if (ctx->stage[a].pending && (rc = stage_sync(ctx, a, a_ms)) != RVCP_OK) return rc;
    if (ctx->stage[b].pending && (rc = stage_sync(ctx, b, b_ms)) != RVCP_OK) return rc;
    return RVCP_OK;
}

static int frame_size_checked(rvcp_ctx_t *ctx, uint32_t width, uint32_t height)
{
    if ((uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "frame too large (W*H must be < 2^31)");
    return RVCP_OK;
}

struct DevRange { const void *p; size_t n; };

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

// A lane of these steps reads its neighbours' pixels, and the frames are not the caller's to
// lose: no output of `step` may overlap an input or another output (NULL ranges overlap nothing)
static int overlap_checked(rvcp_ctx_t *ctx, const char *step, std::initializer_list<DevRange> in,
                           std::initializer_list<DevRange> out)
{
    for (const DevRange *o = out.begin(); o != out.end(); ++o) {
        for (const DevRange &i : in)
            if (ranges_overlap(o->p, o->n, i.p, i.n))
                return fail(ctx, RVCP_E_INVALID, std::string(step) + " output overlaps an input");
        for (const DevRange *q = o + 1; q != out.end(); ++q)
            if (ranges_overlap(o->p, o->n, q->p, q->n))
                return fail(ctx, RVCP_E_INVALID, std::string(step) + " outputs overlap each other");
    }
    return RVCP_OK;
}

// the optional last launch of a step: its linear output as gamma / UNORM8 bytes
static int tonemap_tail(rvcp_ctx_t *ctx, const char *step, const void *d_lin, size_t npx,
                        void *d_rgba8_out, hipStream_t s)
{
    if (d_rgba8_out &&
        rvcp_launch_tonemap((const float *)d_lin, (uint32_t)npx, ctx->d_gamma,
                            (uint32_t *)d_rgba8_out, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string(step) + " tone-map launch failed");
    return RVCP_OK;
}

// ---- G-buffer and denoiser ---------------------------------------------

static int impl_render_gbuffer_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                                     uint32_t width, uint32_t height, void *d_gbuffer, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !d_gbuffer || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid G-buffer arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, "the G-buffer is implemented for the games101 integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "the G-buffer drives one GPU (n_gpus = 1)");
    if (!ctx->has_scene) return fail(ctx, RVCP_E_NO_SCENE, "G-buffer before rvcp_upload_scene");
    if (!primary_t_range_ok(*push, width, height))
        return fail(ctx, RVCP_E_INVALID, "camera t_far x t_coef must stay below 2^24 (the "
                    "shader's miss test t_max + 1, :287, :424)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    primary_frame_args(ctx, *push, width, height, A);
    A.shard_index = 0;
    A.shard_count = 1;
    A.n_pixels = width * height;
    if (rvcp_launch_gbuffer(&A, ctx->d_tri, ctx->d_shade, ctx->d_bvh_nodes, ctx->d_bvh_tris,
                            d_gbuffer, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("G-buffer launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return RVCP_OK;
}

static int impl_denoise_params_default(rvcp_denoise_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    // the best row on average of tools/denoise_sweep.py
    params->iterations = 2;
    params->normal_power_log2 = 7;
    params->sigma_color = INFINITY;
    params->sigma_plane = 0.1f;
    return RVCP_OK;
}

// sigma_i^2 of pass i: sigma_i = sigma_color 2^-i (an exact scaling), squared with one rounding
static float denoise_color_s2(float sigma_color, uint32_t i)
{
    const float sig = sigma_color * std::ldexp(1.0f, -(int)i);
    return sig * sig;
}

static int impl_denoise_async(rvcp_ctx_t *ctx, const void *d_in, const void *d_gbuffer,
                              uint32_t width, uint32_t height, const rvcp_denoise_params_t *params,
                              void *d_out, void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_in || !d_gbuffer || !d_out || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid denoise arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    rvcp_denoise_params_t P;
    if (params) P = *params;
    else (void)impl_denoise_params_default(&P);
    if (P.iterations < 1 || P.iterations > RVCP_DENOISE_MAX_ITERATIONS)
        return fail(ctx, RVCP_E_INVALID, "denoise iterations must be in 1..8");
    if (P.normal_power_log2 > 8)
        return fail(ctx, RVCP_E_INVALID, "denoise normal_power_log2 must be in 0..8");
    const bool use_color = !std::isinf(P.sigma_color);
    // (negated compares: a NaN sigma is rejected too)
    if (!(P.sigma_color > 0.0f) || !(P.sigma_plane > 0.0f))
        return fail(ctx, RVCP_E_INVALID, "denoise sigma_color and sigma_plane must be > 0");
    // the last pass's sigma_i^2 is the smallest: it must not underflow (a zero divisor)
    if (use_color && !(denoise_color_s2(P.sigma_color, P.iterations - 1) >= FLT_MIN))
        return fail(ctx, RVCP_E_INVALID, "denoise sigma_color is too small (sigma_i^2 underflows)");
    const size_t npx = (size_t)width * height;
    // the output must not overlap the input: a pass reads neighbours it would have overwritten
    // (a text of its own, older than overlap_checked's)
    if (ranges_overlap(d_out, npx * 12, d_in, npx * 12))
        return fail(ctx, RVCP_E_INVALID, "denoise output overlaps the input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // intermediates: none for one pass, one buffer for two, both from three passes on
    for (uint32_t b = 0; b < 2 && b + 1 < P.iterations; ++b)
        if ((rc = grow(ctx, (void **)&ctx->d_dn[b], &ctx->cap_dn[b], npx, 12)) != RVCP_OK) return rc;
    if ((rc = stage_begin(ctx, ST_DENOISE, s)) != RVCP_OK) return rc;
    const float *src = (const float *)d_in;
    for (uint32_t i = 0; i < P.iterations; ++i) {
        float *dst = i + 1 == P.iterations ? (float *)d_out : ctx->d_dn[i & 1u];
        if (rvcp_launch_denoise_pass(src, d_gbuffer, dst, width, height, 1u << i,
                                     P.normal_power_log2, use_color ? 1u : 0u,
                                     use_color ? denoise_color_s2(P.sigma_color, i) : 1.0f,
                                     P.sigma_plane, s) != 0)
            return fail(ctx, RVCP_E_HIP, std::string("denoise launch failed: ") +
                                             hipGetErrorString(hipGetLastError()));
        src = dst;
    }
    if ((rc = tonemap_tail(ctx, "denoise", d_out, npx, d_rgba8_out, s)) != RVCP_OK) return rc;
    return stage_end(ctx, ST_DENOISE, s);
}

static int impl_denoise_wait(rvcp_ctx_t *ctx, float *denoise_ms)
{
    return stage_wait(ctx, ST_DENOISE, "no denoise in flight", denoise_ms);
}

// ---- ray queries ---------------------------------------------------------

// the stack of the tree's traversal: kRayQueryLdsStack; the debug build's RVCP_DEBUG_RAYS_LDS=0/1
// chooses per call (the A/B of tools/rays_time.py; the release library holds the kept form only)
static int ray_query_lds_stack()
{
    const char *e = RVCP_KNOB("RVCP_DEBUG_RAYS_LDS");
    return e && (*e == '0' || *e == '1') ? *e - '0' : (kRayQueryLdsStack ? 1 : 0);
}

// what the ray entry points share with rvcp_render_gbuffer_async: a games101 context that drives
// one GPU and holds a scene
static int rays_ctx_checked(rvcp_ctx_t *ctx, const char *what)
{
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, std::string(what) + " is implemented for the games101 integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, std::string(what) + " drives one GPU (n_gpus = 1)");
    if (!ctx->has_scene) return fail(ctx, RVCP_E_NO_SCENE, std::string(what) + " before rvcp_upload_scene");
    return RVCP_OK;
}

// one query enqueued under stage `id` (ST_RAYS: the caller's, ST_RAYS_SYNC: a synchronous call's)
static int trace_rays_enqueue(rvcp_ctx_t *ctx, const void *d_rays, uint32_t n_rays, uint32_t mode,
                              void *d_out, void *stream, StageId id)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_rays || !d_out || n_rays == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid ray query arguments");
    if (n_rays >= (1u << 31))
        return fail(ctx, RVCP_E_INVALID, "too many rays (n_rays must be < 2^31)");
    if (mode != RVCP_RAYS_NEAREST && mode != RVCP_RAYS_ANY)
        return fail(ctx, RVCP_E_INVALID, "ray query mode must be RVCP_RAYS_NEAREST or RVCP_RAYS_ANY");
    if ((uintptr_t)d_rays % 16 || (uintptr_t)d_out % (mode == RVCP_RAYS_ANY ? 4 : 16))
        return fail(ctx, RVCP_E_INVALID, "ray query buffers must be 16-byte aligned (4-byte: the "
                    "RVCP_RAYS_ANY output)");
    int rc;
    if ((rc = rays_ctx_checked(ctx, "a ray query")) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    A.n_pixels = n_rays;
    A.n_faces = ctx->n_faces;
    A.accel = resolved_accel(ctx->cfg.accel, ctx->n_faces);
    A.bvh_root = ctx->bvh_root;
    A.bvh_n4 = ctx->bvh_n4;
    A.bvh_slots = ctx->bvh_slots;
    A.bvh_prefix = A.accel == RVCP_ACCEL_BVH ? ctx->bvh_prefix : 0u;
    if ((rc = stage_begin(ctx, id, s)) != RVCP_OK) return rc;
    if (rvcp_launch_ray_query(&A, ctx->d_tri, ctx->d_bvh_nodes, ctx->d_bvh_tris, d_rays,
                              mode == RVCP_RAYS_ANY, ray_query_lds_stack(), d_out, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("ray query launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, id, s);
}

static int impl_trace_rays_async(rvcp_ctx_t *ctx, const void *d_rays, uint32_t n_rays,
                                 uint32_t mode, void *d_out, void *stream)
{
    return trace_rays_enqueue(ctx, d_rays, n_rays, mode, d_out, stream, ST_RAYS);
}

static int impl_rays_wait(rvcp_ctx_t *ctx, float *rays_ms)
{
    return stage_wait(ctx, ST_RAYS, "no ray query in flight", rays_ms);
}

// the primary rays of pixels [first, first + count) of the W x H frame (the public call: all)
static int primary_rays_launch(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                               uint32_t height, uint32_t first, uint32_t count, void *d_rays,
                               hipStream_t s)
{
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if ((rc = rays_ctx_checked(ctx, "the primary rays' call")) != RVCP_OK) return rc;
    if (!primary_t_range_ok(*push, width, height))
        return fail(ctx, RVCP_E_INVALID, "camera t_far x t_coef must stay below 2^24 (the "
                    "shader's miss test t_max + 1, :287, :424)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    primary_frame_args(ctx, *push, width, height, A);
    A.shard_index = 0;
    A.shard_count = 1;
    A.n_pixels = width * height;
    if (rvcp_launch_primary_rays(&A, first, count, d_rays, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("primary rays launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return RVCP_OK;
}

static int impl_primary_rays_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                                   uint32_t width, uint32_t height, void *d_rays, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !d_rays || width == 0 || height == 0 || (uintptr_t)d_rays % 16)
        return fail(ctx, RVCP_E_INVALID, "invalid primary rays arguments (d_rays: 16-byte aligned)");
    return primary_rays_launch(ctx, push, width, height, 0, width * height, d_rays,
                               stream ? (hipStream_t)stream : ctx->stream);
}

static int impl_trace_rays(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, uint32_t n_rays, uint32_t mode,
                           void *out, float *rays_ms)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!rays || !out || n_rays == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid ray query arguments");
    if (n_rays >= (1u << 31))
        return fail(ctx, RVCP_E_INVALID, "too many rays (n_rays must be < 2^31)");
    if (mode != RVCP_RAYS_NEAREST && mode != RVCP_RAYS_ANY)
        return fail(ctx, RVCP_E_INVALID, "ray query mode must be RVCP_RAYS_NEAREST or RVCP_RAYS_ANY");
    int rc;
    if ((rc = rays_ctx_checked(ctx, "a ray query")) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (the staging is free: only the synchronous calls use it, and each waits for its query)
    const size_t out_elem = mode == RVCP_RAYS_ANY ? sizeof(uint32_t) : sizeof(rvcp_ray_hit_t);
    if ((rc = grow(ctx, &ctx->d_q_rays, &ctx->cap_q_rays, n_rays, sizeof(rvcp_ray_t))) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_q_out, &ctx->cap_q_out, n_rays, sizeof(rvcp_ray_hit_t))) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->d_q_rays, rays, (size_t)n_rays * sizeof(rvcp_ray_t),
                           hipMemcpyHostToDevice));
    if ((rc = trace_rays_enqueue(ctx, ctx->d_q_rays, n_rays, mode, ctx->d_q_out, ctx->stream,
                                 ST_RAYS_SYNC)) != RVCP_OK)
        return rc;
    if ((rc = stage_sync(ctx, ST_RAYS_SYNC, rays_ms)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_q_out, (size_t)n_rays * out_elem, hipMemcpyDeviceToHost));
    return RVCP_OK;
}

static int impl_pick(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                     uint32_t height, uint32_t x, uint32_t y, rvcp_ray_hit_t *out_hit)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !out_hit || width == 0 || height == 0 || x >= width || y >= height)
        return fail(ctx, RVCP_E_INVALID, "invalid pick arguments (x < width, y < height)");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if ((rc = rays_ctx_checked(ctx, "a pick")) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = grow(ctx, &ctx->d_q_rays, &ctx->cap_q_rays, 1, sizeof(rvcp_ray_t))) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_q_out, &ctx->cap_q_out, 1, sizeof(rvcp_ray_hit_t))) != RVCP_OK) return rc;
    if ((rc = primary_rays_launch(ctx, push, width, height, y * width + x, 1, ctx->d_q_rays,
                                  ctx->stream)) != RVCP_OK)
        return rc;
    if ((rc = trace_rays_enqueue(ctx, ctx->d_q_rays, 1, RVCP_RAYS_NEAREST, ctx->d_q_out, ctx->stream,
                                 ST_RAYS_SYNC)) != RVCP_OK)
        return rc;
    if ((rc = stage_sync(ctx, ST_RAYS_SYNC, nullptr)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy(out_hit, ctx->d_q_out, sizeof(*out_hit), hipMemcpyDeviceToHost));
    return RVCP_OK;
}

// ---- path queries --------------------------------------------------------

constexpr size_t kPathCounterWords = 4;     // traversals, queue head, wave iterations, unused

// the counter words of a path query under stage `id`
static unsigned long long *path_counters(rvcp_ctx_t *ctx, StageId id)
{
    return ctx->d_p_counters + (id == ST_PATHS_SYNC ? kPathCounterWords : 0);
}

// the debug build's RVCP_DEBUG_PATHS_STATIC=1: one static ray per lane instead of the queue (the
// A/B of tools/paths_time.py, §4.20; the product library runs the kept form only)
static int path_query_static_lanes()
{
    const char *e = RVCP_KNOB("RVCP_DEBUG_PATHS_STATIC");
    return e && *e == '1' ? 1 : 0;
}

// what the argument checks of the asynchronous and the synchronous call share
static int trace_paths_checked(rvcp_ctx_t *ctx, const void *rays, const void *seeds,
                               uint32_t n_rays, uint32_t spp, const void *out)
{
    if (!rays || !seeds || !out || n_rays == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid path query arguments");
    if (n_rays >= (1u << 31))
        return fail(ctx, RVCP_E_INVALID, "too many rays (n_rays must be < 2^31)");
    if (spp < 1 || spp > RVCP_SPP_MAP_MAX)
        return fail(ctx, RVCP_E_INVALID, "spp must be in 1..256");
    int rc;
    if ((rc = rays_ctx_checked(ctx, "a path query")) != RVCP_OK) return rc;
    if (ctx->sampling == RVCP_SAMPLING_COSINE)
        return fail(ctx, RVCP_E_UNSUPPORTED, "a path query is implemented for the uniform bounce "
                    "(RVCP_SAMPLING_UNIFORM)");
    return RVCP_OK;
}

// one query enqueued under stage `id` (ST_PATHS: the caller's, ST_PATHS_SYNC: rvcp_trace_paths')
static int trace_paths_enqueue(rvcp_ctx_t *ctx, const void *d_rays, const void *d_seeds,
                               uint32_t n_rays, uint32_t spp, void *d_out, void *stream, StageId id)
{
    if (!ctx) return RVCP_E_INVALID;
    int rc;
    if ((rc = trace_paths_checked(ctx, d_rays, d_seeds, n_rays, spp, d_out)) != RVCP_OK) return rc;
    if ((uintptr_t)d_rays % 16 || (uintptr_t)d_seeds % 4 || (uintptr_t)d_out % 4)
        return fail(ctx, RVCP_E_INVALID, "path query buffers must be aligned (rays: 16 bytes, "
                    "seeds and output: 4)");
    if ((rc = overlap_checked(ctx, "a path query",
                              {{d_rays, (size_t)n_rays * sizeof(rvcp_ray_t)},
                               {d_seeds, (size_t)n_rays * sizeof(float)}},
                              {{d_out, (size_t)n_rays * 3 * sizeof(float)}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_p_counters) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_p_counters,
                               2 * kPathCounterWords * sizeof(unsigned long long)));
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    A.n_pixels = n_rays;
    A.spp = spp;
    A.n_faces = ctx->n_faces;
    A.accel = resolved_accel(ctx->cfg.accel, ctx->n_faces);
    A.bvh_root = ctx->bvh_root;
    A.bvh_n4 = ctx->bvh_n4;
    A.bvh_slots = ctx->bvh_slots;
    A.bvh_prefix = A.accel == RVCP_ACCEL_BVH ? ctx->bvh_prefix : 0u;
    shading_frame_args(ctx, A);
    A.n_mats = ctx->n_mats;
    A.n_simds = ctx->n_simds;
    A.shard_count = 1;
    unsigned long long *counters = path_counters(ctx, id);
    if ((rc = stage_begin(ctx, id, s)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(counters, 0, kPathCounterWords * sizeof(unsigned long long), s));
    // with material scattering (rvcp_set_materials, §4.21) its kernel, whatever the scene holds
    const int launch_rc = ctx->materials == RVCP_MATERIALS_SCATTER
        ? rvcp_launch_path_scatter(&A, ctx->d_tri, ctx->d_shade, ctx->d_mats, ctx->d_rawmats,
                                   ctx->d_lights, ctx->d_bvh_nodes, ctx->d_bvh_tris, d_rays,
                                   d_seeds, d_out, counters, ctx->cfg.grid_waves_per_simd, s)
        : rvcp_launch_path_query(&A, ctx->d_tri, ctx->d_shade, ctx->d_mats, ctx->d_lights,
                                 ctx->d_bvh_nodes, ctx->d_bvh_tris, d_rays, d_seeds, d_out, counters,
                                 ctx->cfg.grid_waves_per_simd, path_query_static_lanes(), s);
    if (launch_rc != 0)
        return fail(ctx, RVCP_E_HIP, std::string("path query launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, id, s);
}

// the traversals a finished query under stage `id` made
static int paths_traversals(rvcp_ctx_t *ctx, StageId id, uint64_t *traversals)
{
    if (!traversals) return RVCP_OK;
    unsigned long long t = 0;
    HIP_TRY(ctx, hipMemcpy(&t, path_counters(ctx, id), sizeof(t), hipMemcpyDeviceToHost));
    *traversals = t;
    return RVCP_OK;
}

static int impl_trace_paths_async(rvcp_ctx_t *ctx, const void *d_rays, const void *d_seeds,
                                  uint32_t n_rays, uint32_t spp, void *d_out, void *stream)
{
    return trace_paths_enqueue(ctx, d_rays, d_seeds, n_rays, spp, d_out, stream, ST_PATHS);
}

static int impl_paths_wait(rvcp_ctx_t *ctx, float *paths_ms, uint64_t *traversals)
{
    int rc;
    if ((rc = stage_wait(ctx, ST_PATHS, "no path query in flight", paths_ms)) != RVCP_OK) return rc;
    return paths_traversals(ctx, ST_PATHS, traversals);
}

static int impl_trace_paths(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, const float *seeds,
                            uint32_t n_rays, uint32_t spp, float *out, float *paths_ms,
                            uint64_t *traversals)
{
    if (!ctx) return RVCP_E_INVALID;
    int rc;
    if ((rc = trace_paths_checked(ctx, rays, seeds, n_rays, spp, out)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (the staging is free: only this call uses it, and it waits for its query)
    if ((rc = grow(ctx, &ctx->d_p_rays, &ctx->cap_p_rays, n_rays, sizeof(rvcp_ray_t))) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_p_seeds, &ctx->cap_p_seeds, n_rays, sizeof(float))) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_p_out, &ctx->cap_p_out, n_rays, 3 * sizeof(float))) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->d_p_rays, rays, (size_t)n_rays * sizeof(rvcp_ray_t),
                           hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_p_seeds, seeds, (size_t)n_rays * sizeof(float),
                           hipMemcpyHostToDevice));
    if ((rc = trace_paths_enqueue(ctx, ctx->d_p_rays, ctx->d_p_seeds, n_rays, spp, ctx->d_p_out,
                                  ctx->stream, ST_PATHS_SYNC)) != RVCP_OK)
        return rc;
    if ((rc = stage_sync(ctx, ST_PATHS_SYNC, paths_ms)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_p_out, (size_t)n_rays * 3 * sizeof(float),
                           hipMemcpyDeviceToHost));
    return paths_traversals(ctx, ST_PATHS_SYNC, traversals);
}

static int impl_primary_seeds_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push,
                                    uint32_t width, uint32_t height, void *d_seeds, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !d_seeds || width == 0 || height == 0 || (uintptr_t)d_seeds % 4)
        return fail(ctx, RVCP_E_INVALID, "invalid primary seeds arguments (d_seeds: 4-byte aligned)");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if ((rc = rays_ctx_checked(ctx, "the primary seeds' call")) != RVCP_OK) return rc;
    if (!primary_t_range_ok(*push, width, height))
        return fail(ctx, RVCP_E_INVALID, "camera t_far x t_coef must stay below 2^24 (the "
                    "shader's miss test t_max + 1, :287, :424)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    primary_frame_args(ctx, *push, width, height, A);
    A.shard_index = 0;
    A.shard_count = 1;
    A.n_pixels = width * height;
    if (rvcp_launch_primary_seeds(&A, width * height, d_seeds,
                                  stream ? (hipStream_t)stream : ctx->stream) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("primary seeds launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return RVCP_OK;
}

// ---- temporal reprojection and accumulation -----------------------------

static int impl_temporal_params_default(rvcp_temporal_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    params->alpha_min = 0.05f;
    params->max_history = 32;
    params->sigma_plane = 0.1f;       // the denoiser's plane-distance width
    params->normal_min = 0.9f;
    return RVCP_OK;
}

// *out = *params or the defaults, validated (negated compares: a NaN is rejected too)
static int temporal_params_checked(rvcp_ctx_t *ctx, const rvcp_temporal_params_t *params,
                                   rvcp_temporal_params_t *out)
{
    if (params) *out = *params;
    else (void)impl_temporal_params_default(out);
    if (!(out->alpha_min >= 0.0f && out->alpha_min <= 1.0f))
        return fail(ctx, RVCP_E_INVALID, "temporal alpha_min must be in 0..1");
    if (out->max_history < 1 || out->max_history > RVCP_TEMPORAL_MAX_HISTORY)
        return fail(ctx, RVCP_E_INVALID, "temporal max_history must be in 1..65535");
    if (!(out->sigma_plane > 0.0f))
        return fail(ctx, RVCP_E_INVALID, "temporal sigma_plane must be > 0");
    if (!(out->normal_min >= -1.0f && out->normal_min <= 1.0f))
        return fail(ctx, RVCP_E_INVALID, "temporal normal_min must be in -1..1");
    return RVCP_OK;
}

// The camera as the kernel projects through it, the inverse of sample_ray
// (ray_tracer_games101_branch.comp:217-235), in double: f = forward (ff = |f|^2), r =
// normalize(forward x up) (its u), d = forward x r of length dl (its v: down the image), and a
// pixel centre lies at slope (px + 1/2 - W/2) / k, k = H / (2 tan(vfov/2 * PI/180)), in both
// directions (w = h W / H).  rvcp_temporal_view_from_push and rvcp_taa_jitter_push must agree on
// it bit for bit.
struct CameraBasis { double f[3], r[3], d[3], dl, ff, k; };

// false: forward is zero or parallel to up
static bool camera_basis(const rvcp_camera_t &c, uint32_t height, CameraBasis *b)
{
    const double up[3] = {c.up[0], c.up[1], c.up[2]};
    double *f = b->f, *r = b->r, *d = b->d;
    for (int i = 0; i < 3; ++i) f[i] = c.forward[i];
    r[0] = f[1] * up[2] - f[2] * up[1];
    r[1] = f[2] * up[0] - f[0] * up[2];
    r[2] = f[0] * up[1] - f[1] * up[0];
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    b->ff = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
    if (!(rl > 0.0) || !(b->ff > 0.0)) return false;
    for (int i = 0; i < 3; ++i) r[i] /= rl;
    d[0] = f[1] * r[2] - f[2] * r[1];
    d[1] = f[2] * r[0] - f[0] * r[2];
    d[2] = f[0] * r[1] - f[1] * r[0];
    b->dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(b->dl > 0.0)) return false;
    const double PI = 3.1415926;      // the shader's constant (:15)
    b->k = (double)height / (2.0 * std::tan((double)c.vertical_fov / 2.0 * PI / 180.0));
    return true;
}

// The camera of `push` as a view record: each output rounded once.
static int impl_temporal_view_from_push(const rvcp_push_constant_t *push, uint32_t width,
                                        uint32_t height, rvcp_temporal_view_t *out)
{
    if (!push || !out || width == 0 || height == 0) return RVCP_E_INVALID;
    CameraBasis b;
    if (!camera_basis(push->camera, height, &b)) return RVCP_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < 3; ++i) {
        out->position[i] = push->camera.position[i];
        out->right[i] = (float)b.r[i];
        out->down[i] = (float)(b.d[i] / b.dl);
        out->forward[i] = (float)(b.f[i] / b.ff);
    }
    out->k = (float)b.k;
    return RVCP_OK;
}

static int impl_temporal_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                                          const void *d_cur, const void *d_cur_g,
                                          const void *d_prev, const void *d_prev_g,
                                          const void *d_prev_len, uint32_t width, uint32_t height,
                                          const rvcp_temporal_params_t *params, void *d_out,
                                          void *d_out_len, void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_cur || !d_cur_g || !d_out || !d_out_len || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid temporal arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    const int n_prev = (d_prev ? 1 : 0) + (d_prev_g ? 1 : 0) + (d_prev_len ? 1 : 0);
    if (n_prev != 0 && n_prev != 3)
        return fail(ctx, RVCP_E_INVALID, "temporal history needs d_prev_linear, d_prev_gbuffer "
                    "and d_prev_len together");
    rvcp_temporal_params_t P;
    if ((rc = temporal_params_checked(ctx, params, &P)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "temporal",
                              {{d_cur, npx * 12}, {d_cur_g, npx * 32}, {d_prev, npx * 12},
                               {d_prev_g, npx * 32}, {d_prev_len, npx * 4}},
                              {{d_out, npx * 12}, {d_out_len, npx * 4}, {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_TEMPORAL, s)) != RVCP_OK) return rc;
    const uint32_t mode = n_prev == 0 ? 0u : view ? 2u : 1u;
    if (rvcp_launch_temporal((const float *)d_cur, d_cur_g, (const float *)d_prev, d_prev_g,
                             (const uint32_t *)d_prev_len, (float *)d_out, (uint32_t *)d_out_len,
                             width, height, mode, view, &P, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("temporal launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    if ((rc = tonemap_tail(ctx, "temporal", d_out, npx, d_rgba8_out, s)) != RVCP_OK) return rc;
    return stage_end(ctx, ST_TEMPORAL, s);
}

static int impl_temporal_wait(rvcp_ctx_t *ctx, float *temporal_ms)
{
    return stage_wait(ctx, ST_TEMPORAL, "no temporal step in flight", temporal_ms);
}

static int impl_temporal_reset(rvcp_ctx_t *ctx)
{
    if (!ctx) return RVCP_E_INVALID;
    ctx->tp_hist.valid = false;
    return RVCP_OK;
}

// ---- temporal anti-aliasing: jitter and resolve --------------------------

static int impl_taa_params_default(rvcp_taa_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    params->alpha_min = 0.1f;
    params->max_history = 32;
    params->clamp = 1;
    params->_pad = 0;
    return RVCP_OK;
}

// the radical inverse of i in base b (exact sums of a few negative powers in double)
static double halton(uint32_t i, uint32_t b)
{
    double f = 1.0, r = 0.0;
    while (i > 0) {
        f /= (double)b;
        r += f * (double)(i % b);
        i /= b;
    }
    return r;
}

static int impl_taa_jitter(uint32_t frame_index, float out_jitter[2])
{
    if (!out_jitter) return RVCP_E_INVALID;
    const uint32_t i = frame_index % RVCP_TAA_JITTER_PERIOD + 1u;
    out_jitter[0] = (float)(halton(i, 2) - 0.5);
    out_jitter[1] = (float)(halton(i, 3) - 0.5);
    return RVCP_OK;
}

// The camera of impl_temporal_view_from_push with its forward turned by jitter / k towards right
// and down, keeping its length.  Everything in double, each output rounded once.
static int impl_taa_jitter_push(const rvcp_push_constant_t *base, uint32_t width, uint32_t height,
                                const float jitter[2], rvcp_push_constant_t *out)
{
    if (!base || !jitter || !out || width == 0 || height == 0) return RVCP_E_INVALID;
    // (negated compares: a NaN is rejected too)
    if (!(jitter[0] >= -1.0f && jitter[0] <= 1.0f && jitter[1] >= -1.0f && jitter[1] <= 1.0f))
        return RVCP_E_INVALID;
    CameraBasis b;
    if (!camera_basis(base->camera, height, &b)) return RVCP_E_INVALID;
    const rvcp_push_constant_t copy = *base;        // (out may be base)
    *out = copy;
    if (jitter[0] == 0.0f && jitter[1] == 0.0f) return RVCP_OK;
    const double fl = std::sqrt(b.ff), jx = (double)jitter[0] / b.k, jy = (double)jitter[1] / b.k;
    double n[3];
    for (int i = 0; i < 3; ++i) n[i] = b.f[i] / fl + b.r[i] * jx + (b.d[i] / b.dl) * jy;
    const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int i = 0; i < 3; ++i) out->camera.forward[i] = (float)(n[i] / nl * fl);
    return RVCP_OK;
}

static int impl_taa_resolve_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *cur_view,
                                  const rvcp_temporal_view_t *prev_view, const void *d_cur,
                                  const void *d_cur_g, const void *d_prev, const void *d_prev_len,
                                  uint32_t width, uint32_t height, const rvcp_taa_params_t *params,
                                  void *d_out, void *d_out_len, void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_cur || !d_cur_g || !d_out || !d_out_len || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid TAA resolve arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if ((d_prev == nullptr) != (d_prev_len == nullptr))
        return fail(ctx, RVCP_E_INVALID, "TAA history needs d_prev_resolved and d_prev_len together");
    if ((cur_view == nullptr) != (prev_view == nullptr))
        return fail(ctx, RVCP_E_INVALID, "TAA resolve needs both views or neither");
    rvcp_taa_params_t P;
    if (params) P = *params;
    else (void)impl_taa_params_default(&P);
    // (negated compares: a NaN is rejected too)
    if (!(P.alpha_min >= 0.0f && P.alpha_min <= 1.0f))
        return fail(ctx, RVCP_E_INVALID, "TAA alpha_min must be in 0..1");
    if (P.max_history < 1 || P.max_history > RVCP_TEMPORAL_MAX_HISTORY)
        return fail(ctx, RVCP_E_INVALID, "TAA max_history must be in 1..65535");
    if (P.clamp > 1)
        return fail(ctx, RVCP_E_INVALID, "TAA clamp must be 0 or 1");
    if (P._pad != 0)
        return fail(ctx, RVCP_E_INVALID, "TAA params._pad must be 0");
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "TAA",
                              {{d_cur, npx * 12}, {d_cur_g, npx * 32}, {d_prev, npx * 12},
                               {d_prev_len, npx * 4}},
                              {{d_out, npx * 12}, {d_out_len, npx * 4}, {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_TAA, s)) != RVCP_OK) return rc;
    // a camera at rest fetches q = p exactly and never resamples: byte-equal views are no views
    const bool moved = cur_view && std::memcmp(cur_view, prev_view, sizeof(*cur_view)) != 0;
    const uint32_t mode = !d_prev ? 0u : moved ? 2u : 1u;
    if (rvcp_launch_taa_resolve((const float *)d_cur, d_cur_g, (const float *)d_prev,
                                (const uint32_t *)d_prev_len, (float *)d_out, (uint32_t *)d_out_len,
                                (uint32_t *)d_rgba8_out, ctx->d_gamma, width, height, mode, cur_view,
                                prev_view, &P, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("TAA resolve launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, ST_TAA, s);
}

static int impl_taa_wait(rvcp_ctx_t *ctx, float *taa_ms)
{
    return stage_wait(ctx, ST_TAA, "no TAA resolve in flight", taa_ms);
}

static int impl_set_taa(rvcp_ctx_t *ctx, int on)
{
    if (!ctx) return RVCP_E_INVALID;
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    const bool want = on != 0;
    if (want == ctx->taa) return RVCP_OK;
    ctx->taa = want;
    // histories of centred and of jittered frames do not mix
    ctx->tp_hist.valid = ctx->sv_hist.valid = false;
    ctx->taa_tp.hist.valid = ctx->taa_sv.hist.valid = false;
    return RVCP_OK;
}

static int impl_get_taa(rvcp_ctx_t *ctx, int *on)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!on) return fail(ctx, RVCP_E_INVALID, "invalid get_taa arguments");
    *on = ctx->taa ? 1 : 0;
    return RVCP_OK;
}

// ---- bounce sampling: the switch -------------------------------------------

// the temporal, SVGF, TAA and upsampling histories, dropped when the frames' integrand changes
static void drop_chain_histories(rvcp_ctx_t *ctx)
{
    ctx->tp_hist.valid = ctx->sv_hist.valid = false;
    ctx->taa_tp.hist.valid = ctx->taa_sv.hist.valid = false;
    ctx->taau_tp.hist.valid = ctx->taau_sv.hist.valid = false;
}

static int impl_set_sampling(rvcp_ctx_t *ctx, int32_t sampling)
{
    if (!ctx) return RVCP_E_INVALID;
    if (sampling != RVCP_SAMPLING_UNIFORM && sampling != RVCP_SAMPLING_COSINE)
        return fail(ctx, RVCP_E_INVALID, "unknown sampling");
    if (sampling == RVCP_SAMPLING_COSINE && ctx->cfg.integrator == RVCP_INTEGRATOR_LEGACY)
        return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_SAMPLING_COSINE is for the games101 integrator "
                    "(mode 2's diffuse scatter is cosine-weighted already)");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    for (rvcp_ctx *sub : ctx->subs)
        if (sub->pending)
            return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    if (sampling == RVCP_SAMPLING_COSINE && ctx->materials == RVCP_MATERIALS_SCATTER)
        return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_SAMPLING_COSINE is not implemented with "
                    "RVCP_MATERIALS_SCATTER (its kernel holds the uniform bounce only)");
    if (sampling == ctx->sampling) return RVCP_OK;
    ctx->sampling = sampling;
    for (rvcp_ctx *sub : ctx->subs) sub->sampling = sampling;
    // histories of frames with another expectation and another noise do not mix
    drop_chain_histories(ctx);
    return RVCP_OK;
}

// ---- material scattering: the switch ----------------------------------------

static int impl_set_materials(rvcp_ctx_t *ctx, int32_t materials)
{
    if (!ctx) return RVCP_E_INVALID;
    if (materials != RVCP_MATERIALS_LAMBERTIAN && materials != RVCP_MATERIALS_SCATTER)
        return fail(ctx, RVCP_E_INVALID, "unknown materials mode");
    if (materials == RVCP_MATERIALS_SCATTER) {
        if (ctx->cfg.integrator == RVCP_INTEGRATOR_LEGACY)
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER is for the games101 "
                        "integrator (mode 2 scatters by material already)");
        if (!ctx->subs.empty())
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER drives one GPU (n_gpus = 1)");
        if (ctx->sampling == RVCP_SAMPLING_COSINE)
            return fail(ctx, RVCP_E_UNSUPPORTED, "RVCP_MATERIALS_SCATTER is not implemented with "
                        "RVCP_SAMPLING_COSINE (its kernel holds the uniform bounce only)");
    }
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    if (materials == ctx->materials) return RVCP_OK;
    std::string why;
    if (materials == RVCP_MATERIALS_SCATTER && ctx->has_scene &&
        !scatter_materials_ok(ctx->h_rawmats.data(), (uint32_t)ctx->h_rawmats.size(), why))
        return fail(ctx, RVCP_E_INVALID, why);
    ctx->materials = materials;
    // histories of frames of another integrand do not mix
    drop_chain_histories(ctx);
    return RVCP_OK;
}

static int impl_get_materials(rvcp_ctx_t *ctx, int32_t *materials)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!materials) return fail(ctx, RVCP_E_INVALID, "invalid get_materials arguments");
    *materials = ctx->materials;
    return RVCP_OK;
}

static int impl_get_sampling(rvcp_ctx_t *ctx, int32_t *sampling)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!sampling) return fail(ctx, RVCP_E_INVALID, "invalid get_sampling arguments");
    *sampling = ctx->sampling;
    return RVCP_OK;
}

static int impl_taa_reset(rvcp_ctx_t *ctx)
{
    if (!ctx) return RVCP_E_INVALID;
    ctx->taa_tp.hist.valid = ctx->taa_sv.hist.valid = false;
    ctx->taau_tp.hist.valid = ctx->taau_sv.hist.valid = false;
    return RVCP_OK;
}

// ---- temporal upsampling: the step and the switch -------------------------

static int impl_taau_params_default(rvcp_taau_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    params->max_weight = 8.0f;
    params->init_weight = 0.1f;
    params->clamp = 1;
    params->_pad = 0;
    return RVCP_OK;
}

static int impl_taa_upsample_async(rvcp_ctx_t *ctx, uint32_t scale,
                                   const rvcp_temporal_view_t *jit_view,
                                   const rvcp_temporal_view_t *cur_view,
                                   const rvcp_temporal_view_t *prev_view, const void *d_cur,
                                   const void *d_g_hi, const void *d_prev, const void *d_prev_wt,
                                   uint32_t width, uint32_t height,
                                   const rvcp_taau_params_t *params, void *d_out, void *d_out_wt,
                                   void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!jit_view || !cur_view || !d_cur || !d_out || !d_out_wt || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid TAA upsampling arguments");
    if (scale < 2 || scale > 4)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling scale must be in 2..4");
    if (width % scale != 0 || height % scale != 0)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling: the scale must divide width and height");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if ((d_prev == nullptr) != (d_prev_wt == nullptr))
        return fail(ctx, RVCP_E_INVALID,
                    "TAA upsampling history needs d_prev_resolved and d_prev_weight together");
    if (prev_view && !d_prev)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling: prev_view without a history");
    // a camera at rest fetches q = p exactly and never resamples: byte-equal views are no view
    const bool moved = prev_view && std::memcmp(cur_view, prev_view, sizeof(*cur_view)) != 0;
    if (moved && !d_g_hi)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling: a moved camera needs d_gbuffer_hi");
    rvcp_taau_params_t P;
    if (params) P = *params;
    else (void)impl_taau_params_default(&P);
    // (negated compares: a NaN is rejected too)
    if (!(P.max_weight > 0.0f && P.max_weight <= FLT_MAX))
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling max_weight must be finite and > 0");
    if (!(P.init_weight > 0.0f && P.init_weight <= FLT_MAX))
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling init_weight must be finite and > 0");
    if (P.clamp > 1)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling clamp must be 0 or 1");
    if (P._pad != 0)
        return fail(ctx, RVCP_E_INVALID, "TAA upsampling params._pad must be 0");
    const size_t npx = (size_t)width * height, lpx = npx / scale / scale;
    if ((rc = overlap_checked(ctx, "TAA upsampling",
                              {{d_cur, lpx * 12}, {d_g_hi, npx * 32}, {d_prev, npx * 12},
                               {d_prev_wt, npx * 4}},
                              {{d_out, npx * 12}, {d_out_wt, npx * 4}, {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_TAAU, s)) != RVCP_OK) return rc;
    const uint32_t mode = !d_prev ? 0u : moved ? 2u : 1u;
    if (rvcp_launch_taa_upsample((const float *)d_cur, d_g_hi, (const float *)d_prev,
                                 (const float *)d_prev_wt, (float *)d_out, (float *)d_out_wt,
                                 (uint32_t *)d_rgba8_out, ctx->d_gamma, width, height, scale, mode,
                                 jit_view, cur_view, prev_view, &P, 0u, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("TAA upsampling launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, ST_TAAU, s);
}

static int impl_taau_wait(rvcp_ctx_t *ctx, float *taau_ms)
{
    return stage_wait(ctx, ST_TAAU, "no TAA upsampling step in flight", taau_ms);
}

static int impl_set_taa_upsample(rvcp_ctx_t *ctx, uint32_t scale)
{
    if (!ctx) return RVCP_E_INVALID;
    if (scale < 1 || scale > 4)
        return fail(ctx, RVCP_E_INVALID, "the TAA upsampling scale must be in 1..4");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    if (scale == ctx->taau_scale) return RVCP_OK;
    ctx->taau_scale = scale;
    // histories of frames traced at different sizes do not mix
    ctx->tp_hist.valid = ctx->sv_hist.valid = false;
    ctx->taa_tp.hist.valid = ctx->taa_sv.hist.valid = false;
    ctx->taau_tp.hist.valid = ctx->taau_sv.hist.valid = false;
    return RVCP_OK;
}

static int impl_get_taa_upsample(rvcp_ctx_t *ctx, uint32_t *scale)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!scale) return fail(ctx, RVCP_E_INVALID, "invalid get_taa_upsample arguments");
    *scale = ctx->taau_scale;
    return RVCP_OK;
}

// ---- SVGF: moments, variance and the variance-guided filter --------------

static int impl_svgf_params_default(rvcp_svgf_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    // the best row of tools/svgf_sweep.py; spatial_below ties there and takes the SVGF paper's 4
    // 
    params->iterations = 3;
    params->normal_power_log2 = 7;    // the denoiser's
    params->sigma_luminance = 1.0f;
    params->sigma_plane = 0.1f;       // the denoiser's plane-distance width
    params->epsilon = 1.0e-4f;        // the square of a 1 % luminance step
    params->alpha_moments_min = 0.05f;    // the colour's alpha_min
    params->spatial_below = 4;
    params->_pad = 0;
    return RVCP_OK;
}

// *out = *params or the defaults, validated (negated compares: a NaN is rejected too)
static int svgf_params_checked(rvcp_ctx_t *ctx, const rvcp_svgf_params_t *params,
                               rvcp_svgf_params_t *out)
{
    if (params) *out = *params;
    else (void)impl_svgf_params_default(out);
    if (out->iterations < 1 || out->iterations > RVCP_SVGF_MAX_ITERATIONS)
        return fail(ctx, RVCP_E_INVALID, "svgf iterations must be in 1..8");
    if (out->normal_power_log2 > 8)
        return fail(ctx, RVCP_E_INVALID, "svgf normal_power_log2 must be in 0..8");
    if (!(out->sigma_luminance > 0.0f) || !(out->sigma_plane > 0.0f) || !(out->epsilon > 0.0f))
        return fail(ctx, RVCP_E_INVALID, "svgf sigma_luminance, sigma_plane and epsilon must be > 0");
    if (!(out->alpha_moments_min >= 0.0f && out->alpha_moments_min <= 1.0f))
        return fail(ctx, RVCP_E_INVALID, "svgf alpha_moments_min must be in 0..1");
    if (out->spatial_below < 1 || out->spatial_below > RVCP_SVGF_MAX_SPATIAL_BELOW)
        return fail(ctx, RVCP_E_INVALID, "svgf spatial_below must be in 1..16");
    if (out->_pad != 0) return fail(ctx, RVCP_E_INVALID, "svgf _pad must be 0");
    return RVCP_OK;
}

static int impl_svgf_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                                      const void *d_cur, const void *d_cur_g, const void *d_prev,
                                      const void *d_prev_g, const void *d_prev_len,
                                      const void *d_prev_m, uint32_t width, uint32_t height,
                                      const rvcp_temporal_params_t *tparams,
                                      const rvcp_svgf_params_t *sparams, void *d_out,
                                      void *d_out_len, void *d_out_m, void *d_rgba8_out,
                                      void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_cur || !d_cur_g || !d_out || !d_out_len || !d_out_m || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid svgf accumulation arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    const int n_prev = (d_prev ? 1 : 0) + (d_prev_g ? 1 : 0) + (d_prev_len ? 1 : 0) + (d_prev_m ? 1 : 0);
    if (n_prev != 0 && n_prev != 4)
        return fail(ctx, RVCP_E_INVALID, "svgf history needs d_prev_linear, d_prev_gbuffer, "
                    "d_prev_len and d_prev_moments together");
    rvcp_temporal_params_t P;
    if ((rc = temporal_params_checked(ctx, tparams, &P)) != RVCP_OK) return rc;
    rvcp_svgf_params_t S;
    if ((rc = svgf_params_checked(ctx, sparams, &S)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "svgf accumulation",
                              {{d_cur, npx * 12}, {d_cur_g, npx * 32}, {d_prev, npx * 12},
                               {d_prev_g, npx * 32}, {d_prev_len, npx * 4}, {d_prev_m, npx * 8}},
                              {{d_out, npx * 12}, {d_out_len, npx * 4}, {d_out_m, npx * 8},
                               {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_SVGF_ACC, s)) != RVCP_OK) return rc;
    const uint32_t mode = n_prev == 0 ? 0u : view ? 2u : 1u;
    if (rvcp_launch_svgf_temporal((const float *)d_cur, d_cur_g, (const float *)d_prev, d_prev_g,
                                  (const uint32_t *)d_prev_len, (const float *)d_prev_m,
                                  (float *)d_out, (uint32_t *)d_out_len, (float *)d_out_m, width,
                                  height, mode, view, &P, S.alpha_moments_min, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("svgf accumulation launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    if ((rc = tonemap_tail(ctx, "svgf accumulation", d_out, npx, d_rgba8_out, s)) != RVCP_OK)
        return rc;
    return stage_end(ctx, ST_SVGF_ACC, s);
}

static int impl_svgf_filter_async(rvcp_ctx_t *ctx, const void *d_lin, const void *d_mom,
                                  const void *d_len, const void *d_gbuffer, uint32_t width,
                                  uint32_t height, const rvcp_svgf_params_t *params, void *d_out,
                                  void *d_var_out, void *d_fb_out, void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_lin || !d_mom || !d_len || !d_gbuffer || !d_out || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid svgf filter arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    rvcp_svgf_params_t P;
    if ((rc = svgf_params_checked(ctx, params, &P)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "svgf filter",
                              {{d_lin, npx * 12}, {d_mom, npx * 8}, {d_len, npx * 4},
                               {d_gbuffer, npx * 32}},
                              {{d_out, npx * 12}, {d_var_out, npx * 4}, {d_fb_out, npx * 12},
                               {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // variance: the estimate in plane 0, pass i from plane i & 1 into the other one; colour
    // intermediates from two passes on (pass 0 may write the caller's feedback buffer instead)
    for (uint32_t b = 0; b < 2; ++b)
        if ((rc = grow(ctx, (void **)&ctx->d_sv_var[b], &ctx->cap_sv_var[b], npx, 4)) != RVCP_OK)
            return rc;
    for (uint32_t b = 0; b < 2 && b + 1 < P.iterations; ++b)
        if ((rc = grow(ctx, (void **)&ctx->d_sv_tmp[b], &ctx->cap_sv_tmp[b], npx, 12)) != RVCP_OK)
            return rc;
    if ((rc = stage_begin(ctx, ST_SVGF_FLT, s)) != RVCP_OK) return rc;
    if (rvcp_launch_svgf_variance((const float *)d_mom, (const uint32_t *)d_len, d_gbuffer,
                                  ctx->d_sv_var[0], width, height, P.spatial_below,
                                  P.normal_power_log2, P.sigma_plane, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("svgf variance launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    const bool use_lum = !std::isinf(P.sigma_luminance);
    const float sigma_l2 = use_lum ? P.sigma_luminance * P.sigma_luminance : 1.0f;
    const float *src = (const float *)d_lin;
    for (uint32_t i = 0; i < P.iterations; ++i) {
        const bool last = i + 1 == P.iterations;
        float *dst = last ? (float *)d_out
                          : (i == 0 && d_fb_out) ? (float *)d_fb_out : ctx->d_sv_tmp[i & 1u];
        float *vdst = last && d_var_out ? (float *)d_var_out : ctx->d_sv_var[(i + 1u) & 1u];
        if (rvcp_launch_svgf_pass(src, ctx->d_sv_var[i & 1u], d_gbuffer, dst, vdst, width, height,
                                  1u << i, P.normal_power_log2, use_lum ? 1u : 0u, sigma_l2,
                                  P.epsilon, P.sigma_plane, 0u, s) != 0)
            return fail(ctx, RVCP_E_HIP, std::string("svgf pass launch failed: ") +
                                             hipGetErrorString(hipGetLastError()));
        src = dst;
    }
    if (d_fb_out && P.iterations == 1)          // pass 0 is the last pass
        HIP_TRY(ctx, hipMemcpyAsync(d_fb_out, d_out, npx * 12, hipMemcpyDeviceToDevice, s));
    if ((rc = tonemap_tail(ctx, "svgf", d_out, npx, d_rgba8_out, s)) != RVCP_OK) return rc;
    return stage_end(ctx, ST_SVGF_FLT, s);
}

static int impl_svgf_wait(rvcp_ctx_t *ctx, float *accumulate_ms, float *filter_ms)
{
    return stage_wait2(ctx, ST_SVGF_ACC, ST_SVGF_FLT, "no svgf step in flight", accumulate_ms,
                       filter_ms);
}

static int impl_svgf_reset(rvcp_ctx_t *ctx)
{
    if (!ctx) return RVCP_E_INVALID;
    ctx->sv_hist.valid = false;
    return RVCP_OK;
}

// ---- albedo demodulation --------------------------------------------------

// what both steps check before anything is enqueued (the restrictions of the G-buffer)
static int albedo_checked(rvcp_ctx_t *ctx, uint32_t width, uint32_t height)
{
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, "the G-buffer is implemented for the games101 integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "albedo demodulation drives one GPU (n_gpus = 1)");
    if (!ctx->has_scene)
        return fail(ctx, RVCP_E_NO_SCENE, "albedo demodulation before rvcp_upload_scene");
    return RVCP_OK;
}

static int impl_demodulate_async(rvcp_ctx_t *ctx, const void *d_lin, const void *d_gbuffer,
                                 uint32_t width, uint32_t height, void *d_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_lin || !d_gbuffer || !d_out || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid demodulate arguments");
    int rc;
    if ((rc = albedo_checked(ctx, width, height)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    // a lane reads and writes its own pixel only: exactly in place is legal, a partial overlap
    // is not
    if (ranges_overlap(d_out, npx * 12, d_gbuffer, npx * 32) ||
        (d_out != d_lin && ranges_overlap(d_out, npx * 12, d_lin, npx * 12)))
        return fail(ctx, RVCP_E_INVALID, "demodulate output overlaps an input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_DEMOD, s)) != RVCP_OK) return rc;
    if (rvcp_launch_demodulate((const float *)d_lin, d_gbuffer, ctx->d_albedo, ctx->n_mats,
                               (float *)d_out, (uint32_t)npx, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("demodulate launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, ST_DEMOD, s);
}

static int impl_remodulate_async(rvcp_ctx_t *ctx, const void *d_irr, const void *d_gbuffer,
                                 uint32_t width, uint32_t height, void *d_lin_out,
                                 void *d_rgba8_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_irr || !d_gbuffer || (!d_lin_out && !d_rgba8_out) || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid remodulate arguments");
    int rc;
    if ((rc = albedo_checked(ctx, width, height)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "remodulate", {{d_irr, npx * 12}, {d_gbuffer, npx * 32}},
                              {{d_lin_out, npx * 12}, {d_rgba8_out, npx * 4}})) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = stage_begin(ctx, ST_REMOD, s)) != RVCP_OK) return rc;
    if (rvcp_launch_remodulate((const float *)d_irr, d_gbuffer, ctx->d_albedo, ctx->n_mats,
                               ctx->d_gamma, (float *)d_lin_out, (uint32_t *)d_rgba8_out,
                               (uint32_t)npx, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("remodulate launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, ST_REMOD, s);
}

static int impl_albedo_wait(rvcp_ctx_t *ctx, float *demodulate_ms, float *remodulate_ms)
{
    return stage_wait2(ctx, ST_DEMOD, ST_REMOD, "no albedo step in flight", demodulate_ms,
                       remodulate_ms);
}

static int impl_set_demodulation(rvcp_ctx_t *ctx, int on)
{
    if (!ctx) return RVCP_E_INVALID;
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    const bool want = on != 0;
    if (want == ctx->demodulation) return RVCP_OK;
    ctx->demodulation = want;
    // colour histories and irradiance histories do not mix
    ctx->tp_hist.valid = ctx->sv_hist.valid = false;
    return RVCP_OK;
}

static int impl_get_demodulation(rvcp_ctx_t *ctx, int *on)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!on) return fail(ctx, RVCP_E_INVALID, "invalid get_demodulation arguments");
    *on = ctx->demodulation ? 1 : 0;
    return RVCP_OK;
}

// ---- adaptive sampling: the plan step and the switch -----------------------

static int impl_adaptive_params_default(rvcp_adaptive_params_t *params)
{
    if (!params) return RVCP_E_INVALID;
    // the best row on average of tools/adaptive_sweep.py
    params->spp_min = 1;
    params->spp_max = 32;
    params->mean_spp = 4.0f;
    params->weight_cap = 0.0625f;
    params->epsilon = 1e-2f;
    params->_pad = 0;
    return RVCP_OK;
}

// *out = *params or the defaults, validated (negated compares: a NaN is rejected too)
static int adaptive_params_checked(rvcp_ctx_t *ctx, const rvcp_adaptive_params_t *params,
                                   rvcp_adaptive_params_t *out)
{
    if (params) *out = *params;
    else (void)impl_adaptive_params_default(out);
    if (out->spp_min < 1 || out->spp_min > RVCP_SPP_MAP_MAX)
        return fail(ctx, RVCP_E_INVALID, "adaptive spp_min must be in 1..256");
    if (out->spp_max < out->spp_min || out->spp_max > RVCP_SPP_MAP_MAX)
        return fail(ctx, RVCP_E_INVALID, "adaptive spp_max must be in spp_min..256");
    if (!(out->mean_spp >= (float)out->spp_min && out->mean_spp <= (float)out->spp_max))
        return fail(ctx, RVCP_E_INVALID, "adaptive mean_spp must be in spp_min..spp_max");
    if (!(out->weight_cap > 0.0f && out->weight_cap < INFINITY))
        return fail(ctx, RVCP_E_INVALID, "adaptive weight_cap must be finite and > 0");
    if (!(out->epsilon > 0.0f && out->epsilon < INFINITY))
        return fail(ctx, RVCP_E_INVALID, "adaptive epsilon must be finite and > 0");
    if (out->_pad != 0) return fail(ctx, RVCP_E_INVALID, "adaptive params._pad must be 0");
    return RVCP_OK;
}

static int impl_spp_plan_async(rvcp_ctx_t *ctx, const void *d_variance, const void *d_linear,
                               const void *d_len, const void *d_gbuffer, uint32_t width,
                               uint32_t height, const rvcp_adaptive_params_t *params,
                               void *d_map_out, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_variance || !d_linear || !d_gbuffer || !d_map_out || width == 0 || height == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid plan arguments");
    int rc;
    if ((rc = frame_size_checked(ctx, width, height)) != RVCP_OK) return rc;
    rvcp_adaptive_params_t P;
    if ((rc = adaptive_params_checked(ctx, params, &P)) != RVCP_OK) return rc;
    const size_t npx = (size_t)width * height;
    if ((rc = overlap_checked(ctx, "plan",
                              {{d_variance, npx * 4}, {d_linear, npx * 12}, {d_len, npx * 4},
                               {d_gbuffer, npx * 32}},
                              {{d_map_out, npx * 4}})) != RVCP_OK)
        return rc;
    // the budget B = floor(mean_spp npx) and what it leaves above spp_min for every pixel (mean_spp
    // >= spp_min; the max is against the rounding of the product)
    const uint64_t budget = (uint64_t)std::floor((double)P.mean_spp * (double)npx);
    const uint64_t floor_px = (uint64_t)P.spp_min * npx;
    const uint64_t extra = budget > floor_px ? budget - floor_px : 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = grow(ctx, (void **)&ctx->d_ad_q, &ctx->cap_ad_q, npx, 4)) != RVCP_OK) return rc;
    if (!ctx->d_ad_sums) HIP_TRY(ctx, hipMalloc((void **)&ctx->d_ad_sums, 2 * sizeof(unsigned long long)));
    if ((rc = stage_begin(ctx, ST_PLAN, s)) != RVCP_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ad_sums, 0, 2 * sizeof(unsigned long long), s));
    if (rvcp_launch_spp_plan((const float *)d_variance, (const float *)d_linear,
                             (const uint32_t *)d_len, d_gbuffer, (uint32_t)npx, P.weight_cap,
                             P.epsilon, P.spp_min, P.spp_max, extra, ctx->d_ad_q, ctx->d_ad_sums,
                             (uint32_t *)d_map_out, s) != 0)
        return fail(ctx, RVCP_E_HIP, std::string("plan launch failed: ") +
                                         hipGetErrorString(hipGetLastError()));
    return stage_end(ctx, ST_PLAN, s);
}

static int impl_spp_plan_wait(rvcp_ctx_t *ctx, float *plan_ms, uint64_t *planned_samples)
{
    int rc;
    if ((rc = stage_wait(ctx, ST_PLAN, "no plan step in flight", plan_ms)) != RVCP_OK) return rc;
    if (planned_samples) {
        unsigned long long sums[2] = {};
        HIP_TRY(ctx, hipMemcpy(sums, ctx->d_ad_sums, sizeof(sums), hipMemcpyDeviceToHost));
        *planned_samples = sums[1];
    }
    return RVCP_OK;
}

static int impl_set_adaptive(rvcp_ctx_t *ctx, const rvcp_adaptive_params_t *params)
{
    if (!ctx) return RVCP_E_INVALID;
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, "adaptive sampling is implemented for the games101 "
                    "integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, "adaptive sampling drives one GPU (n_gpus = 1)");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    if (params) {
        rvcp_adaptive_params_t P;
        const int rc = adaptive_params_checked(ctx, params, &P);
        if (rc != RVCP_OK) return rc;
        ctx->ad_params = P;
    }
    ctx->adaptive = params != nullptr;
    ctx->ad_valid = false;      // the map is dropped; the SVGF history is not
    return RVCP_OK;
}

static int impl_get_adaptive(rvcp_ctx_t *ctx, int *on, rvcp_adaptive_params_t *out_params)
{
    if (!ctx) return RVCP_E_INVALID;
    if (on) *on = ctx->adaptive ? 1 : 0;
    if (out_params) {
        if (ctx->adaptive) *out_params = ctx->ad_params;
        else (void)impl_adaptive_params_default(out_params);
    }
    return RVCP_OK;
}

static int impl_adaptive_last_map(rvcp_ctx_t *ctx, uint32_t *out_map, uint32_t *out_width,
                                  uint32_t *out_height)
{
    if (!ctx) return RVCP_E_INVALID;
    if (ctx->ad_last < 0) return fail(ctx, RVCP_E_INVALID, "no frame was traced through a map yet");
    if (out_width) *out_width = ctx->ad_w;
    if (out_height) *out_height = ctx->ad_h;
    if (out_map) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpy(out_map, ctx->d_ad_map[ctx->ad_last], (size_t)ctx->ad_w * ctx->ad_h * 4,
                               hipMemcpyDeviceToHost));
    }
    return RVCP_OK;
}

// ---- the chains: rvcp_render_denoised, rvcp_render_temporal, rvcp_render_svgf ----------------

// What a stateful chain does for its resolve state `st` before it renders (the TAA switch is set,
// or the upsampling scale is above 1: with_gbuf).  width x height is the size of the state's
// frames (the OUTPUT size when upsampling), lw x lh the traced frame's, whose jitter this is;
// `have` says whether the chain's own history continues.  *jpush becomes the jittered push of
// this frame, *resume whether the resolve has a history.
static int resolve_begin(rvcp_ctx_t *ctx, ResolveState &st, bool with_gbuf, bool have,
                         const rvcp_push_constant_t *push, uint32_t width, uint32_t height,
                         uint32_t lw, uint32_t lh, rvcp_push_constant_t *jpush, bool *resume)
{
    int rc;
    if ((rc = reserve_resolve_state(ctx, st, (size_t)width * height, with_gbuf)) != RVCP_OK)
        return rc;
    *resume = have && st.hist.continues_at(width, height);
    if (!*resume) st.counter = 0;       // the state is dropped with the chain's history
    st.hist.valid = false;              // until this frame is complete
    float j[2];
    (void)impl_taa_jitter(st.counter, j);
    if (impl_taa_jitter_push(push, lw, lh, j, jpush) != RVCP_OK)
        return fail(ctx, RVCP_E_INVALID, "the camera's forward is zero or parallel to up");
    return RVCP_OK;
}

// ... and behind its last step, with the TAA switch: the resolve of d_final under the unjittered
// cameras into the state's free slot and d_rgba
static int taa_chain_resolve(rvcp_ctx_t *ctx, ResolveState &st, bool resume,
                             const rvcp_push_constant_t *push, const rvcp_temporal_view_t *base_view,
                             const float *d_final, const void *d_gbuffer, uint32_t width,
                             uint32_t height)
{
    const uint32_t prev = st.hist.slot, cur = prev ^ 1u;
    const bool at_rest = resume &&
                         std::memcmp(&st.hist.camera, &push->camera, sizeof(rvcp_camera_t)) == 0;
    return impl_taa_resolve_async(ctx, at_rest ? nullptr : base_view,
                                  at_rest ? nullptr : &st.hist.view, d_final, d_gbuffer,
                                  resume ? st.d_res[prev] : nullptr,
                                  resume ? st.d_aux[prev] : nullptr, width, height, nullptr,
                                  st.d_res[cur], st.d_aux[cur], ctx->d_rgba, ctx->stream);
}

// ... or, with the upsampling scale: the output-size G-buffer through the unjittered camera when
// it moved, and the upsampling of d_final (traced through jit_view) into the state's free slot
// and d_rgba
static int taau_chain_resolve(rvcp_ctx_t *ctx, ResolveState &st, bool resume,
                              const rvcp_push_constant_t *push, const rvcp_temporal_view_t *base_view,
                              const rvcp_temporal_view_t *jit_view, const float *d_final,
                              uint32_t width, uint32_t height)
{
    const uint32_t prev = st.hist.slot, cur = prev ^ 1u;
    const bool moved = resume &&
                       std::memcmp(&st.hist.camera, &push->camera, sizeof(rvcp_camera_t)) != 0;
    if (moved) {
        const int rc = impl_render_gbuffer_async(ctx, push, width, height, st.d_gbuf, ctx->stream);
        if (rc != RVCP_OK) return rc;
    }
    return impl_taa_upsample_async(ctx, ctx->taau_scale, jit_view, base_view,
                                   moved ? &st.hist.view : nullptr, d_final,
                                   moved ? st.d_gbuf : nullptr, resume ? st.d_res[prev] : nullptr,
                                   resume ? st.d_aux[prev] : nullptr, width, height, nullptr,
                                   st.d_res[cur], st.d_aux[cur], ctx->d_rgba, ctx->stream);
}

// The per-frame locals of a chain.  A chain is: render (the raw linear frame), G-buffer
// [, demodulate in place], its own one or two steps [, remodulate] [, resolve or upsampling], in
// this order on the context's stream; the last RGBA8 store overwrites the render's.
struct ChainFrame {
    const char *name = "";                          // for the error texts
    const rvcp_push_constant_t *base_push = nullptr;    // the caller's camera
    const rvcp_push_constant_t *push = nullptr;     // what the chain renders through (or &jpush)
    rvcp_push_constant_t jpush;
    // With the upsampling scale `up` above 1 (§4.14): width x height is the TRACED frame, the
    // whole chain runs at that size, and out_w x out_h is what the last step writes
    uint32_t up = 1, width = 0, height = 0, out_w = 0, out_h = 0;
    size_t npx = 0, out_npx = 0;
    rvcp_temporal_view_t view_now = {};             // of push, at the traced size
    rvcp_temporal_view_t base_view = {};            // of base_push, at the output size
    bool have = false;              // the chain's own history continues
    bool same_camera = false;       // ... and needs no reprojection
    // With the demodulation switch set (§4.12): the raw frame is demodulated in place right after
    // the G-buffer, histories and filters are in irradiance and store nothing, and the fused
    // remodulate + store writes the colour into the raw frame's buffer (free by then) and the
    // RGBA8 frame.
    bool demod = false;
    // With the TAA switch set (§4.13), rs = the chain's state of it: everything runs through the
    // jittered camera jpush, the chain's own history always reprojects (through the jittered
    // cameras), no step stores RGBA8, and the resolve of the final linear colour under the
    // unjittered cameras ends the frame.  With the upsampling scale above 1 the upsampling step
    // takes the resolve's place.
    ResolveState *rs = nullptr;
    bool resume = false;            // the resolve has a history
    uint32_t *store = nullptr;      // the chain's own RGBA8 store
    uint32_t enqueued = 0;          // stage_bit()s of the own steps the chain has enqueued
};

// what every chain checks first
static int chain_args_checked(rvcp_ctx_t *ctx, const char *name, const rvcp_push_constant_t *push,
                              const uint8_t *out_rgba8, uint32_t width, uint32_t height,
                              bool bad_flags)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!push || !out_rgba8 || width == 0 || height == 0 ||
        (uint64_t)width * height >= (1ull << 31) || bad_flags)
        return fail(ctx, RVCP_E_INVALID, std::string("invalid ") + name + " arguments");
    if (ctx->cfg.integrator != RVCP_INTEGRATOR_GAMES101)
        return fail(ctx, RVCP_E_UNSUPPORTED, "the G-buffer is implemented for the games101 integrator");
    if (!ctx->subs.empty())
        return fail(ctx, RVCP_E_UNSUPPORTED, std::string(name) + " drives one GPU (n_gpus = 1)");
    if (ctx->pending)
        return fail(ctx, RVCP_E_INVALID, "a frame is in flight on this context (rvcp_wait first)");
    return RVCP_OK;
}

static int chain_bad_camera(rvcp_ctx_t *ctx, const ChainFrame &F)
{
    return fail(ctx, RVCP_E_INVALID,
                std::string(F.name) + ": the camera's forward is zero or parallel to up");
}

// A stateful chain's frame: the sizes, the camera's view, the device and the RGBA8 staging
static int chain_begin(rvcp_ctx_t *ctx, ChainFrame &F, const char *name,
                       const rvcp_push_constant_t *push, uint32_t width, uint32_t height)
{
    F.name = name;
    F.base_push = F.push = push;
    F.up = ctx->taau_scale;
    F.out_w = width;
    F.out_h = height;
    if (F.up > 1) {
        if (width % F.up != 0 || height % F.up != 0)
            return fail(ctx, RVCP_E_INVALID, std::string(name) +
                        ": the TAA upsampling scale must divide width and height");
        width /= F.up;
        height /= F.up;
    }
    F.width = width;
    F.height = height;
    if (impl_temporal_view_from_push(push, width, height, &F.view_now) != RVCP_OK)
        return chain_bad_camera(ctx, F);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    F.npx = (size_t)width * height;
    F.out_npx = (size_t)F.out_w * F.out_h;
    return grow(ctx, (void **)&ctx->d_rgba, &ctx->cap_rgba, F.out_npx, 4);
}

// ... and, once the chain's buffers hold F.npx pixels, what continues: the chain's history `hist`
// and, with the TAA switch or the upsampling scale, its state of that (taa_st / taau_st), whose
// jittered camera the frame is then rendered through.  Both are invalid until chain_commit.
static int chain_history(rvcp_ctx_t *ctx, ChainFrame &F, History &hist, ResolveState &taa_st,
                         ResolveState &taau_st)
{
    F.have = hist.continues_at(F.width, F.height);
    F.demod = ctx->demodulation;
    F.base_view = F.view_now;
    if (F.up > 1 &&
        impl_temporal_view_from_push(F.base_push, F.out_w, F.out_h, &F.base_view) != RVCP_OK)
        return chain_bad_camera(ctx, F);
    if (ctx->taa || F.up > 1) {
        F.rs = F.up > 1 ? &taau_st : &taa_st;
        const int rc = resolve_begin(ctx, *F.rs, F.up > 1, F.have, F.base_push, F.out_w, F.out_h,
                                     F.width, F.height, &F.jpush, &F.resume);
        if (rc != RVCP_OK) return rc;
        F.push = &F.jpush;
        if (impl_temporal_view_from_push(F.push, F.width, F.height, &F.view_now) != RVCP_OK)
            return chain_bad_camera(ctx, F);
    }
    F.same_camera = !F.rs && F.have &&
                    std::memcmp(&hist.camera, &F.push->camera, sizeof(rvcp_camera_t)) == 0;
    F.store = F.rs ? nullptr : ctx->d_rgba;
    hist.valid = false;
    return RVCP_OK;
}

// Behind the render of the raw frame into d_cur: the G-buffer [and the demodulation in place]
static int chain_gbuffer(rvcp_ctx_t *ctx, const ChainFrame &F, float *d_cur, void *d_gbuf)
{
    int rc = impl_render_gbuffer_async(ctx, F.push, F.width, F.height, d_gbuf, ctx->stream);
    if (rc == RVCP_OK && F.demod)
        rc = impl_demodulate_async(ctx, d_cur, d_gbuf, F.width, F.height, d_cur, ctx->stream);
    return rc;
}

// Behind the chain's own steps, which went `rc` and left d_out: [the remodulation into d_cur]
// [and the resolve or the upsampling] of *d_final, the displayed linear frame.  After a failure
// anywhere behind the render the chain waits for what it enqueued -- the render always, its own
// steps if they were, the albedo steps if pending -- so that nothing stays pending, and the first
// error's text is kept.
static int chain_tail(rvcp_ctx_t *ctx, ChainFrame &F, int rc, const float *d_out, const void *d_gbuf,
                      float *d_cur, const float **d_final)
{
    if (rc == RVCP_OK && F.demod)
        rc = impl_remodulate_async(ctx, d_out, d_gbuf, F.width, F.height, d_cur, F.store,
                                   ctx->stream);
    *d_final = F.demod ? d_cur : d_out;
    if (rc == RVCP_OK && F.rs)
        rc = F.up > 1 ? taau_chain_resolve(ctx, *F.rs, F.resume, F.base_push, &F.base_view,
                                           &F.view_now, *d_final, F.out_w, F.out_h)
                      : taa_chain_resolve(ctx, *F.rs, F.resume, F.base_push, &F.base_view, *d_final,
                                          d_gbuf, F.width, F.height);
    if (rc == RVCP_OK) return RVCP_OK;
    const std::string why = ctx->err;
    (void)rvcp_wait(ctx, nullptr);
    if (F.enqueued & stage_bit(ST_TEMPORAL)) (void)impl_temporal_wait(ctx, nullptr);
    if (F.enqueued & stage_bit(ST_DENOISE)) (void)impl_denoise_wait(ctx, nullptr);
    if (F.enqueued & stage_bit(ST_SVGF_ACC)) (void)impl_svgf_wait(ctx, nullptr, nullptr);
    if (ctx->stage[ST_DEMOD].pending || ctx->stage[ST_REMOD].pending)
        (void)impl_albedo_wait(ctx, nullptr, nullptr);
    if (F.enqueued & stage_bit(ST_PLAN)) (void)impl_spp_plan_wait(ctx, nullptr, nullptr);
    ctx->err = why;
    return rc;
}

// Behind the waits for the render and the chain's own steps: those for the albedo steps and the
// resolve, and the frame's copies to the host
static int chain_end(rvcp_ctx_t *ctx, const ChainFrame &F, const float *d_final, uint8_t *out_rgba8,
                     float *out_linear_rgb)
{
    int rc;
    if (F.demod && (rc = impl_albedo_wait(ctx, nullptr, nullptr)) != RVCP_OK) return rc;
    if (F.rs) {
        if ((rc = F.up > 1 ? impl_taau_wait(ctx, nullptr) : impl_taa_wait(ctx, nullptr)) != RVCP_OK)
            return rc;
        d_final = F.rs->d_res[F.rs->hist.slot ^ 1u];
    }
    HIP_TRY(ctx, hipMemcpy(out_rgba8, ctx->d_rgba, F.out_npx * 4, hipMemcpyDeviceToHost));
    if (out_linear_rgb)
        HIP_TRY(ctx, hipMemcpy(out_linear_rgb, d_final, F.out_npx * 12, hipMemcpyDeviceToHost));
    return RVCP_OK;
}

// the frame is complete
static void chain_commit(const ChainFrame &F, History &hist)
{
    hist.commit(F.width, F.height, F.push->camera, F.view_now);
    if (F.rs) {
        F.rs->hist.commit(F.out_w, F.out_h, F.base_push->camera, F.base_view);
        F.rs->counter += 1;
    }
}

static int impl_render_denoised(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                                uint32_t height, const rvcp_denoise_params_t *params,
                                uint8_t *out_rgba8, float *out_linear_rgb, rvcp_stats_t *stats,
                                float *denoise_ms)
{
    int rc;
    if ((rc = chain_args_checked(ctx, "render_denoised", push, out_rgba8, width, height,
                                 false)) != RVCP_OK)
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)width * height;
    if ((rc = grow(ctx, (void **)&ctx->d_rgba, &ctx->cap_rgba, npx, 4)) != RVCP_OK) return rc;
    if ((rc = grow(ctx, &ctx->d_gbuf, &ctx->cap_gbuf, npx, sizeof(rvcp_gbuffer_texel_t))) != RVCP_OK)
        return rc;
    if ((rc = grow(ctx, (void **)&ctx->d_dn_in, &ctx->cap_dn_in, npx, 12)) != RVCP_OK ||
        (rc = grow(ctx, (void **)&ctx->d_dn_out, &ctx->cap_dn_out, npx, 12)) != RVCP_OK)
        return rc;
    ChainFrame F;               // (stateless: no history, no resolve)
    F.push = push;
    F.width = width;
    F.height = height;
    F.out_npx = npx;
    F.demod = ctx->demodulation;
    F.store = ctx->d_rgba;
    if ((rc = rvcp_render_async(ctx, push, width, height, ctx->d_rgba, ctx->d_dn_in, ctx->stream)) != RVCP_OK)
        return rc;
    rc = chain_gbuffer(ctx, F, ctx->d_dn_in, ctx->d_gbuf);
    if (rc == RVCP_OK) {
        rc = impl_denoise_async(ctx, ctx->d_dn_in, ctx->d_gbuf, width, height, params,
                                ctx->d_dn_out, F.demod ? nullptr : F.store, ctx->stream);
        if (rc == RVCP_OK) F.enqueued |= stage_bit(ST_DENOISE);
    }
    const float *d_final;
    if ((rc = chain_tail(ctx, F, rc, ctx->d_dn_out, ctx->d_gbuf, ctx->d_dn_in, &d_final)) != RVCP_OK)
        return rc;
    if ((rc = rvcp_wait(ctx, stats)) != RVCP_OK) return rc;
    if ((rc = impl_denoise_wait(ctx, denoise_ms)) != RVCP_OK) return rc;
    return chain_end(ctx, F, d_final, out_rgba8, out_linear_rgb);
}

static int impl_render_temporal(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                                uint32_t height, const rvcp_temporal_params_t *tparams,
                                uint32_t flags, const rvcp_denoise_params_t *dparams,
                                uint8_t *out_rgba8, float *out_linear_rgb,
                                uint32_t *out_history_len, rvcp_stats_t *stats, float *temporal_ms,
                                float *denoise_ms)
{
    int rc;
    if ((rc = chain_args_checked(ctx, "render_temporal", push, out_rgba8, width, height,
                                 (flags & ~RVCP_TEMPORAL_DENOISE) != 0)) != RVCP_OK)
        return rc;
    ChainFrame F;
    if ((rc = chain_begin(ctx, F, "render_temporal", push, width, height)) != RVCP_OK) return rc;
    const bool denoise = (flags & RVCP_TEMPORAL_DENOISE) != 0;
    if ((rc = reserve_temporal_state(ctx, F.npx)) != RVCP_OK) return rc;
    if (denoise &&
        (rc = grow(ctx, (void **)&ctx->d_tp_show, &ctx->cap_tp_show, F.npx, 12)) != RVCP_OK)
        return rc;
    History &hist = ctx->tp_hist;
    if ((rc = chain_history(ctx, F, hist, ctx->taa_tp, ctx->taau_tp)) != RVCP_OK) return rc;
    const uint32_t prev = hist.slot, cur = prev ^ 1u;
    float *const d_cur = ctx->d_tp_cur, *const d_acc = ctx->d_tp_lin[cur];
    void *const d_gbuf = ctx->d_tp_gbuf[cur];
    if ((rc = rvcp_render_async(ctx, F.push, F.width, F.height, ctx->d_rgba, d_cur, ctx->stream)) != RVCP_OK)
        return rc;
    // accumulation [, filter of the accumulated frame: the history stays unfiltered]
    rc = chain_gbuffer(ctx, F, d_cur, d_gbuf);
    if (rc == RVCP_OK) {
        rc = impl_temporal_accumulate_async(
            ctx, F.same_camera ? nullptr : &hist.view, d_cur, d_gbuf,
            F.have ? ctx->d_tp_lin[prev] : nullptr, F.have ? ctx->d_tp_gbuf[prev] : nullptr,
            F.have ? ctx->d_tp_len[prev] : nullptr, F.width, F.height, tparams, d_acc,
            ctx->d_tp_len[cur], denoise || F.demod ? nullptr : F.store, ctx->stream);
        if (rc == RVCP_OK) F.enqueued |= stage_bit(ST_TEMPORAL);
    }
    if (rc == RVCP_OK && denoise) {
        rc = impl_denoise_async(ctx, d_acc, d_gbuf, F.width, F.height, dparams, ctx->d_tp_show,
                                F.demod ? nullptr : F.store, ctx->stream);
        if (rc == RVCP_OK) F.enqueued |= stage_bit(ST_DENOISE);
    }
    const float *d_final;
    if ((rc = chain_tail(ctx, F, rc, denoise ? ctx->d_tp_show : d_acc, d_gbuf, d_cur,
                         &d_final)) != RVCP_OK)
        return rc;
    if ((rc = rvcp_wait(ctx, stats)) != RVCP_OK) return rc;
    if ((rc = impl_temporal_wait(ctx, temporal_ms)) != RVCP_OK) return rc;
    if (denoise_ms) *denoise_ms = 0.0f;
    if (denoise && (rc = impl_denoise_wait(ctx, denoise_ms)) != RVCP_OK) return rc;
    if ((rc = chain_end(ctx, F, d_final, out_rgba8, out_linear_rgb)) != RVCP_OK) return rc;
    if (out_history_len)
        HIP_TRY(ctx, hipMemcpy(out_history_len, ctx->d_tp_len[cur], F.npx * 4, hipMemcpyDeviceToHost));
    chain_commit(F, hist);
    return RVCP_OK;
}

static int impl_render_svgf(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                            uint32_t height, const rvcp_temporal_params_t *tparams,
                            const rvcp_svgf_params_t *sparams, uint32_t flags, uint8_t *out_rgba8,
                            float *out_linear_rgb, float *out_variance, uint32_t *out_history_len,
                            rvcp_stats_t *stats, float *accumulate_ms, float *filter_ms)
{
    int rc;
    if ((rc = chain_args_checked(ctx, "render_svgf", push, out_rgba8, width, height,
                                 (flags & ~RVCP_SVGF_FEEDBACK) != 0)) != RVCP_OK)
        return rc;
    ChainFrame F;
    if ((rc = chain_begin(ctx, F, "render_svgf", push, width, height)) != RVCP_OK) return rc;
    const bool feedback = (flags & RVCP_SVGF_FEEDBACK) != 0;
    if ((rc = reserve_svgf_state(ctx, F.npx)) != RVCP_OK) return rc;
    History &hist = ctx->sv_hist;
    if ((rc = chain_history(ctx, F, hist, ctx->taa_sv, ctx->taau_sv)) != RVCP_OK) return rc;
    const uint32_t prev = hist.slot, cur = prev ^ 1u;
    float *const d_cur = ctx->d_sv_cur;
    void *const d_gbuf = ctx->d_sv_gbuf[cur];
    // With the adaptive switch (§4.18): the raw frame through the map the previous frame planned,
    // in that frame's pixel grid, while the SVGF history continues; else through a uniform map
    const bool adaptive = ctx->adaptive;
    const rvcp_adaptive_params_t &AP = ctx->ad_params;
    if (adaptive) {
        const bool planned = ctx->ad_valid && F.have && ctx->ad_w == F.width && ctx->ad_h == F.height;
        ctx->ad_valid = false;              // until this frame is complete
        for (int i = 0; i < 2; ++i)
            if ((rc = grow(ctx, (void **)&ctx->d_ad_map[i], &ctx->cap_ad_map[i], F.npx, 4)) != RVCP_OK)
                return rc;
        const uint32_t fl = (uint32_t)AP.mean_spp;     // floor: mean_spp >= 1
        const uint32_t uniform = fl < AP.spp_min ? AP.spp_min : fl > AP.spp_max ? AP.spp_max : fl;
        if (!planned &&
            rvcp_launch_fill_map(ctx->d_ad_map[ctx->ad_slot], (uint32_t)F.npx, uniform, ctx->stream) != 0)
            return fail(ctx, RVCP_E_HIP, "render_svgf: the uniform map's launch failed");
        rc = impl_render_spp_map_async(ctx, F.push, F.width, F.height, ctx->d_ad_map[ctx->ad_slot],
                                       uniform, ctx->d_rgba, d_cur, ctx->stream);
    } else {
        rc = rvcp_render_async(ctx, F.push, F.width, F.height, ctx->d_rgba, d_cur, ctx->stream);
    }
    if (rc != RVCP_OK) return rc;
    // accumulation of colour and moments, then the filter
    rc = chain_gbuffer(ctx, F, d_cur, d_gbuf);
    if (rc == RVCP_OK) {
        rc = impl_svgf_accumulate_async(
            ctx, F.same_camera ? nullptr : &hist.view, d_cur, d_gbuf,
            F.have ? ctx->d_sv_lin[prev] : nullptr, F.have ? ctx->d_sv_gbuf[prev] : nullptr,
            F.have ? ctx->d_sv_len[prev] : nullptr, F.have ? ctx->d_sv_mom[prev] : nullptr, F.width,
            F.height, tparams, sparams, ctx->d_sv_lin[cur], ctx->d_sv_len[cur], ctx->d_sv_mom[cur],
            nullptr, ctx->stream);
        if (rc == RVCP_OK) F.enqueued |= stage_bit(ST_SVGF_ACC);   // (its wait is the filter's too)
    }
    if (rc == RVCP_OK)
        rc = impl_svgf_filter_async(ctx, ctx->d_sv_lin[cur], ctx->d_sv_mom[cur], ctx->d_sv_len[cur],
                                    d_gbuf, F.width, F.height, sparams, ctx->d_sv_show,
                                    ctx->d_sv_showvar, feedback ? ctx->d_sv_fb : nullptr,
                                    F.demod ? nullptr : F.store, ctx->stream);
    // ... and the next frame's map from this frame's filtered colour, variance, lengths and G-buffer
    if (rc == RVCP_OK && adaptive) {
        rc = impl_spp_plan_async(ctx, ctx->d_sv_showvar, ctx->d_sv_show, ctx->d_sv_len[cur], d_gbuf,
                                 F.width, F.height, &AP, ctx->d_ad_map[ctx->ad_slot ^ 1u], ctx->stream);
        if (rc == RVCP_OK) F.enqueued |= stage_bit(ST_PLAN);
    }
    const float *d_final;
    if ((rc = chain_tail(ctx, F, rc, ctx->d_sv_show, d_gbuf, d_cur, &d_final)) != RVCP_OK) return rc;
    if ((rc = rvcp_wait(ctx, stats)) != RVCP_OK) return rc;
    if ((rc = impl_svgf_wait(ctx, accumulate_ms, filter_ms)) != RVCP_OK) return rc;
    if (adaptive && (rc = impl_spp_plan_wait(ctx, nullptr, nullptr)) != RVCP_OK) return rc;
    if ((rc = chain_end(ctx, F, d_final, out_rgba8, out_linear_rgb)) != RVCP_OK) return rc;
    if (out_variance)
        HIP_TRY(ctx, hipMemcpy(out_variance, ctx->d_sv_showvar, F.npx * 4, hipMemcpyDeviceToHost));
    if (out_history_len)
        HIP_TRY(ctx, hipMemcpy(out_history_len, ctx->d_sv_len[cur], F.npx * 4, hipMemcpyDeviceToHost));
    // feedback: the next frame's colour history is pass 0's output (moments and lengths stay)
    if (feedback) std::swap(ctx->d_sv_lin[cur], ctx->d_sv_fb);
    chain_commit(F, hist);
    if (adaptive) {         // the frame's map stays readable; the planned one is the next frame's
        ctx->ad_last = (int)ctx->ad_slot;
        ctx->ad_slot ^= 1u;
        ctx->ad_w = F.width;
        ctx->ad_h = F.height;
        ctx->ad_valid = true;
    }
    return RVCP_OK;
}
static int impl_assemble_frame_async(rvcp_ctx_t *ctx, const void *d_gathered, uint32_t slot_rows,
                              uint32_t width, uint32_t height, uint32_t shard_count,
                              void *d_frame, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!d_gathered || !d_frame || width == 0 || height == 0 || shard_count == 0)
        return fail(ctx, RVCP_E_INVALID, "invalid assemble arguments");
    for (uint32_t k = 0; k < shard_count; k++)
        if (rvcp_shard_rows(height, k, shard_count) > slot_rows)
            return fail(ctx, RVCP_E_INVALID, "slot_rows smaller than a shard");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (rvcp_launch_assemble((const uint32_t *)d_gathered, slot_rows, width, height, shard_count,
                             (uint32_t *)d_frame, s) != 0)
        return fail(ctx, RVCP_E_HIP, "assemble launch failed");
    return RVCP_OK;
}


// ---- one process per GPU: the frame gather over RCCL ----
static int impl_rccl_unique_id(uint8_t *out_id)
{
    if (!out_id) return fail(nullptr, RVCP_E_INVALID, "null id buffer");
    const RcclApi &R = rccl_api();
    if (!R.ok) return fail(nullptr, RVCP_E_UNSUPPORTED, R.why);
    static_assert(sizeof(ncclUniqueId) == RVCP_RCCL_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    const ncclResult_t r = R.get_unique_id(&id);
    if (r != ncclSuccess) return fail(nullptr, RVCP_E_HIP, std::string("ncclGetUniqueId: ") + R.error_string(r));
    std::memcpy(out_id, &id, sizeof(id));
    return RVCP_OK;
}

// debug build only (tools/rccl_timeout_diag.py): stage stamps of the communicator paths on stderr
static void rccl_trace(const char *what, long v = 0)
{
    static const bool on = RVCP_KNOB("RVCP_DEBUG_RCCL_TRACE") != nullptr;
    if (on) std::fprintf(stderr, "rvcp rccl: %s %ld\n", what, v);
}

static Clock::time_point comm_deadline(const rvcp_ctx_t *ctx)
{
    return ctx->comm_timeout_ms ? Clock::now() + std::chrono::milliseconds(ctx->comm_timeout_ms)
                                : Clock::time_point::max();
}

// Abort ctx's communicator (ours) after a deadline or an asynchronous error: ncclCommAbort
// raises RCCL's abort flag, which its kernels poll in every wait loop, so a gather stuck on a
// peer that never comes finishes and the streams drain; the context stays usable for
// single-GPU renders.  The abort itself runs on a detached thread: it also joins RCCL's own
// threads, and a wait for a peer that never comes must not become a wait inside the abort.  A
// caller's communicator (rvcp_rccl_attach) is the caller's to abort.
static void abort_comm(rvcp_ctx_t *ctx)
{
    if (ctx->comm && ctx->comm_owned) {
        const ncclComm_t c = ctx->comm;
        rccl_trace("abort: detached ncclCommAbort");
        auto done = std::make_shared<std::atomic<bool>>(false);
        ctx->aborts.push_back(done);          // rvcp_destroy waits for it (bounded)
        std::thread([c, done] {
            (void)rccl_api().comm_abort(c);
            done->store(true);
        }).detach();
    }
    if (ctx->comm_owned) ctx->comm = nullptr;
}

// A gather that timed out and whose stream did not drain (an attached communicator, which this
// library cannot abort, or an abort that has not taken effect): the context forgets the
// communicator (the caller's stays the caller's to abort), later renders stop waiting for the
// gather (a wait on its end event would never return), the gather stream it sits on is retired
// (a new gather gets a fresh one), and its end event is kept for rvcp_destroy.
static int retire_stuck_gather(rvcp_ctx_t *ctx)
{
    ctx->stuck_gathers.push_back(ctx->evg1);
    ctx->evg1 = nullptr;
    if (ctx->gather_on_gstream && ctx->gstream) {
        ctx->retired_gstreams.push_back(ctx->gstream);
        ctx->gstream = nullptr;
    }
    ctx->gather_on_gstream = false;
    ctx->gather_pending = false;
    ctx->comm = nullptr;
    HIP_TRY(ctx, hipEventCreate(&ctx->evg1));
    return RVCP_OK;
}

// Wait until a non-blocking communicator has finished its last call (ncclInProgress ->
// ncclSuccess), bounded by `deadline`.  RVCP_E_TIMEOUT on expiry, RVCP_E_HIP on an RCCL error.
static int wait_comm_ready(rvcp_ctx_t *ctx, ncclComm_t comm, Clock::time_point deadline,
                           const char *what)
{
    const RcclApi &R = rccl_api();
    for (unsigned spin = 0;; spin++) {
        ncclResult_t st = ncclInProgress;
        const ncclResult_t r = R.get_async_error(comm, &st);
        if (r != ncclSuccess)
            return fail(ctx, RVCP_E_HIP, std::string(what) + ": ncclCommGetAsyncError: " + R.error_string(r));
        if (st == ncclSuccess) return RVCP_OK;
        if (st != ncclInProgress)
            return fail(ctx, RVCP_E_HIP, std::string(what) + ": " + R.error_string(st));
        if (Clock::now() >= deadline)
            return fail(ctx, RVCP_E_TIMEOUT, std::string(what) + ": no progress within " +
                        std::to_string(ctx->comm_timeout_ms) + " ms (a peer rank missing or failed)");
        std::this_thread::sleep_for(std::chrono::microseconds(spin < 100 ? 20 : 1000));
    }
}

// The communicator's creation runs on a worker thread: ncclCommInitRankConfig (blocking = 0)
// and the poll of ncclCommGetAsyncError until the rendezvous completes.  The caller waits for
// the worker with the deadline, so rvcp_rccl_init returns in time whatever RCCL does inside
// (on this image's RCCL 2.27.7 the "non-blocking" ncclCommInitRankConfig itself does not return
// while a peer is absent: profiles/history/r05g_rccl_diag.log, tools/rccl_timeout_diag.py); a worker left
// behind aborts its half-made communicator if it ever gets control back (detached: the process
// never waits for it, and exits cleanly, tests/test_gpu_rccl_timeout.py).
struct CommJob {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclResult_t result = ncclSuccess;
    ncclComm_t comm = nullptr;
};

// Creation workers abandoned at their deadline and still blocked inside RCCL, process-wide
// (reported in the messages: each holds a thread and a half-made communicator until RCCL
// returns, which on RCCL 2.27.7 is never while the peer stays absent)
static std::atomic<int> g_blocked_init_workers{0};

static int impl_rccl_init(rvcp_ctx_t *ctx, const uint8_t *id, uint32_t world, uint32_t rank)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!id || world == 0 || rank >= world || world > 4096)
        return fail(ctx, RVCP_E_INVALID, "invalid RCCL rank / world");
    if (ctx->comm) return fail(ctx, RVCP_E_INVALID, "context already has a communicator");
    if (ctx->init_job) {
        // the worker of this context's last timed-out creation: refuse a new one while it is
        // still blocked inside RCCL (retries must not leak a thread each)
        std::lock_guard<std::mutex> g(ctx->init_job->m);
        if (!ctx->init_job->done)
            return fail(ctx, RVCP_E_BUSY, "rvcp_rccl_init: this context's previous creation timed "
                        "out and its worker is still blocked inside RCCL (" +
                        std::to_string(g_blocked_init_workers.load()) + " such worker(s) in the "
                        "process); use another context, or retry once RCCL has returned");
    }
    ctx->init_job.reset();
    const RcclApi &R = rccl_api();
    if (!R.ok) return fail(ctx, RVCP_E_UNSUPPORTED, R.why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    const Clock::time_point deadline = comm_deadline(ctx);
    auto job = std::make_shared<CommJob>();
    const int dev = ctx->device;
    std::thread([job, uid, world, rank, dev]() mutable {
        const RcclApi &R = rccl_api();
        (void)hipSetDevice(dev);
        // non-blocking: a library older than this header reads only the fields it knows (`size`
        // tells it how many there are)
        ncclConfig_t conf = NCCL_CONFIG_INITIALIZER;
        conf.blocking = 0;
        ncclComm_t comm = nullptr;
        rccl_trace("init worker: calling ncclCommInitRankConfig, world", (long)world);
        ncclResult_t r = R.comm_init_rank_config(&comm, (int)world, uid, (int)rank, &conf);
        rccl_trace("init worker: returned", (long)r);
        for (unsigned spin = 0; r == ncclSuccess || r == ncclInProgress; spin++) {
            ncclResult_t st = ncclInProgress;
            if (!comm || R.get_async_error(comm, &st) != ncclSuccess) { r = ncclInternalError; break; }
            if (st != ncclInProgress) { r = st; break; }
            {
                std::lock_guard<std::mutex> g(job->m);
                if (job->abandoned) break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(spin < 100 ? 20 : 1000));
        }
        bool keep;
        {
            std::lock_guard<std::mutex> g(job->m);
            keep = !job->abandoned && r == ncclSuccess;
            job->result = r;
            if (keep) job->comm = comm;
            job->done = true;
            if (job->abandoned) g_blocked_init_workers--;
        }
        job->cv.notify_all();
        if (!keep && comm) {
            rccl_trace("init worker: ncclCommAbort");
            (void)R.comm_abort(comm);
            rccl_trace("init worker: ncclCommAbort returned");
        }
    }).detach();
    std::unique_lock<std::mutex> lk(job->m);
    bool finished;
    if (ctx->comm_timeout_ms == 0) {
        job->cv.wait(lk, [&] { return job->done; });
        finished = true;
    } else {
        finished = job->cv.wait_until(lk, deadline, [&] { return job->done; });
    }
    if (!finished) {
        job->abandoned = true;
        const int blocked = ++g_blocked_init_workers;
        ctx->init_job = job;
        ctx->comm_timed_out = true;
        rccl_trace("init: deadline, worker abandoned");
        return fail(ctx, RVCP_E_TIMEOUT, "ncclCommInitRankConfig: no rendezvous within " +
                    std::to_string(ctx->comm_timeout_ms) + " ms (a peer rank missing or failed); "
                    "the half-made communicator is aborted once RCCL returns; its creation worker "
                    "is left blocked inside RCCL (" + std::to_string(blocked) + " in the process) "
                    "and this context refuses another rvcp_rccl_init until it returns");
    }
    if (job->result != ncclSuccess)
        return fail(ctx, RVCP_E_HIP, std::string("ncclCommInitRankConfig: ") + R.error_string(job->result));
    ctx->comm = job->comm;
    ctx->comm_owned = true;
    ctx->comm_timed_out = false;
    ctx->comm_world = world;
    ctx->comm_rank = rank;
    return RVCP_OK;
}

static int impl_rccl_set_timeout(rvcp_ctx_t *ctx, uint32_t timeout_ms)
{
    if (!ctx) return RVCP_E_INVALID;
    ctx->comm_timeout_ms = timeout_ms;
    return RVCP_OK;
}

static int impl_rccl_attach(rvcp_ctx_t *ctx, void *nccl_comm, uint32_t world, uint32_t rank)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!nccl_comm || world == 0 || rank >= world)
        return fail(ctx, RVCP_E_INVALID, "invalid communicator / rank / world");
    if (ctx->comm) return fail(ctx, RVCP_E_INVALID, "context already has a communicator");
    if (!rccl_api().ok) return fail(ctx, RVCP_E_UNSUPPORTED, rccl_api().why);
    ctx->comm = (ncclComm_t)nccl_comm;
    ctx->comm_owned = false;
    ctx->comm_timed_out = false;
    ctx->comm_world = world;
    ctx->comm_rank = rank;
    return RVCP_OK;
}

static int impl_gather_frame_async(rvcp_ctx_t *ctx, const void *d_shard_rgba8, uint32_t width,
                                   uint32_t height, void *d_gathered, void *d_frame, void *stream)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->comm && ctx->comm_timed_out)
        return fail(ctx, RVCP_E_TIMEOUT, "the communicator was given up after a gather or creation "
                    "deadline; rvcp_rccl_init / rvcp_rccl_attach a new one first");
    if (!ctx->comm) return fail(ctx, RVCP_E_INVALID, "no communicator (rvcp_rccl_init first)");
    const bool root = ctx->comm_rank == 0;
    if (!d_shard_rgba8 || width == 0 || height == 0 || (root && (!d_gathered || !d_frame)))
        return fail(ctx, RVCP_E_INVALID, "invalid gather arguments");
    if ((uint64_t)width * height >= (1ull << 31))
        return fail(ctx, RVCP_E_INVALID, "frame too large (W*H must be < 2^31)");
    // the gather assumes this rank rendered shard comm_rank of comm_world of this frame size;
    // anything else would assemble a scrambled frame on rank 0
    if (ctx->last_shard_count != ctx->comm_world || ctx->last_shard_index != ctx->comm_rank ||
        ctx->last_width != width || ctx->last_height != height)
        return fail(ctx, RVCP_E_INVALID, "gather after a render of another shard / frame size "
                    "(rvcp_render_shard_async must use shard_index = rank, shard_count = world)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the caller's stream, or the context's gather stream behind the render (evr): the
    // gather and rank 0's assembly then leave the render stream free for the next frame
    if (!stream && !ctx->gstream) {
        // the frame gather's own stream, at the device's highest priority: its RCCL and
        // assembly kernels are dispatched ahead of other streams' queued work
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&ctx->gstream, hipStreamNonBlocking, greatest) != hipSuccess) {
            ctx->gstream = nullptr;
            return fail(ctx, RVCP_E_HIP, "gather stream creation failed");
        }
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->gstream;
    if (!stream) {
        HIP_TRY(ctx, hipEventRecord(ctx->evr, ctx->render_stream ? ctx->render_stream : ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evr, 0));
    }
    const uint32_t N = ctx->comm_world;
    const uint32_t slot = rvcp_shard_rows(height, 0, N);      // shard 0 has the most rows
    HIP_TRY(ctx, hipEventRecord(ctx->evg0, s));
    const ncclResult_t r = rccl_api().gather(d_shard_rgba8, root ? d_gathered : nullptr,
                                             (size_t)slot * width, ncclUint32, 0, ctx->comm, s);
    if (r != ncclSuccess && r != ncclInProgress)
        return fail(ctx, RVCP_E_HIP, std::string("ncclGather: ") + rccl_api().error_string(r));
    if (r == ncclInProgress) {
        // a non-blocking communicator -- ours, or an attached one created with blocking = 0
        // (torch's non-blocking communicators) -- may still be connecting to its peers (first
        // gather): the collective is on stream s only once it has, so the assembly and evg1
        // must not be queued before that; bounded by the deadline
        const int rc = wait_comm_ready(ctx, ctx->comm, comm_deadline(ctx), "ncclGather");
        if (rc != RVCP_OK) {
            // ours is aborted; an attached one only its owner may abort: dropped either way
            abort_comm(ctx);
            ctx->comm = nullptr;
            ctx->comm_timed_out = rc == RVCP_E_TIMEOUT;
            return rc;
        }
    }
    if (root && rvcp_launch_assemble((const uint32_t *)d_gathered, slot, width, height, N,
                                     (uint32_t *)d_frame, s) != 0)
        return fail(ctx, RVCP_E_HIP, "assemble launch failed");
    HIP_TRY(ctx, hipEventRecord(ctx->evg1, s));
    ctx->gather_pending = true;
    ctx->gather_on_gstream = !stream;
    return RVCP_OK;
}

// Poll the gather's end event against the deadline (a hipEventSynchronize would block forever
// when a peer never enters the collective); on expiry, or when RCCL reports an asynchronous
// error, abort the communicator so that the stuck kernel exits and the streams drain.
static int wait_gather_done(rvcp_ctx_t *ctx)
{
    const Clock::time_point deadline = comm_deadline(ctx);
    const RcclApi &R = rccl_api();
    for (unsigned spin = 0;; spin++) {
        const hipError_t q = hipEventQuery(ctx->evg1);
        if (q == hipSuccess) return RVCP_OK;
        if (q != hipErrorNotReady)
            return fail(ctx, RVCP_E_HIP, std::string("gather: ") + hipGetErrorString(q));
        if (ctx->comm && (spin & 63) == 63) {
            ncclResult_t st = ncclSuccess;
            if (R.get_async_error(ctx->comm, &st) == ncclSuccess && st != ncclSuccess &&
                st != ncclInProgress) {
                const std::string msg = std::string("ncclGather: ") + R.error_string(st);
                abort_comm(ctx);
                return fail(ctx, RVCP_E_HIP, msg);
            }
        }
        if (Clock::now() >= deadline) {
            const bool owned = ctx->comm_owned;
            abort_comm(ctx);
            // the aborted kernels exit; give the stream a bounded moment to drain so that the
            // context's buffers are no longer read when the caller frees or reuses them
            const Clock::time_point drain = Clock::now() + std::chrono::seconds(owned ? 5 : 0);
            while (hipEventQuery(ctx->evg1) == hipErrorNotReady && Clock::now() < drain)
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            const bool drained = hipEventQuery(ctx->evg1) == hipSuccess;
            ctx->comm_timed_out = true;
            if (drained) {
                ctx->gather_pending = false;
                ctx->gather_on_gstream = false;
                ctx->comm = nullptr;
            } else {
                const int rc = retire_stuck_gather(ctx);
                if (rc != RVCP_OK) return rc;
            }
            return fail(ctx, RVCP_E_TIMEOUT, "gather not complete within " +
                        std::to_string(ctx->comm_timeout_ms) +
                        " ms (a peer rank missing or failed); " +
                        (owned ? "communicator aborted" : "the attached communicator is dropped "
                                 "(abort it: only its owner can)") +
                        (drained ? "" : "; its stream has not drained: later renders do not wait "
                                        "for it, and a new gather needs a new communicator"));
        }
        std::this_thread::sleep_for(std::chrono::microseconds(spin < 2000 ? 5 : 200));
    }
}

static int impl_gather_wait(rvcp_ctx_t *ctx, float *gather_ms, float *frame_ms)
{
    if (!ctx) return RVCP_E_INVALID;
    if (!ctx->gather_pending) return fail(ctx, RVCP_E_INVALID, "no gather in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = wait_gather_done(ctx);
    if (rc != RVCP_OK) return rc;
    ctx->gather_pending = false;
    float ms = 0.0f;
    if (gather_ms) {
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->evg0, ctx->evg1));
        *gather_ms = ms;
    }
    if (frame_ms) {
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->evg1));
        *frame_ms = ms;
    }
    return RVCP_OK;
}

// ---------------------------------------------------------------------------------------
// Exception barrier: every int-returning entry point runs its implementation inside
// `barrier`, so no C++ exception (std::bad_alloc from a host vector or string, anything a
// runtime library throws) crosses the C-ABI (rvcp.h conventions).
// ---------------------------------------------------------------------------------------

int rvcp_config_default_for(int32_t integrator, rvcp_config_t *cfg)
{
    return barrier(nullptr, [&] { return impl_config_default_for(integrator, cfg); });
}

int rvcp_config_default(rvcp_config_t *cfg)
{
    return barrier(nullptr, [&] { return impl_config_default(cfg); });
}

int rvcp_create(const rvcp_config_t *cfg, rvcp_ctx_t **out_ctx)
{
    return barrier(nullptr, [&] { return impl_create(cfg, out_ctx); });
}

int rvcp_destroy(rvcp_ctx_t *ctx)
{
    return barrier(nullptr, [&] { return impl_destroy(ctx); });
}

int rvcp_upload_scene(rvcp_ctx_t *ctx, const rvcp_material_t *materials, uint32_t n_materials,
                      const rvcp_vertex_t *vertices, uint32_t n_vertices,
                      const rvcp_face_t *faces, uint32_t n_faces,
                      const rvcp_sphere_t *spheres, uint32_t n_spheres,
                      const uint32_t *lum_face_ids, uint32_t n_lum_face_ids,
                      const uint32_t *lum_sphere_ids, uint32_t n_lum_sphere_ids)
{
    return barrier(ctx, [&] { return impl_upload_scene(ctx, materials, n_materials, vertices,
        n_vertices, faces, n_faces, spheres, n_spheres, lum_face_ids, n_lum_face_ids,
        lum_sphere_ids, n_lum_sphere_ids); });
}

int rvcp_upload_scene_file(rvcp_ctx_t *ctx, const char *path, rvcp_camera_t *out_camera)
{
    return barrier(ctx, [&] { return impl_upload_scene_file(ctx, path, out_camera); });
}

int rvcp_render_shard_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                            uint32_t height, uint32_t shard_index, uint32_t shard_count,
                            void *d_rgba8, void *d_linear_rgb, void *stream)
{
    return barrier(ctx, [&] { return impl_render_shard_async(ctx, push, width, height,
        shard_index, shard_count, d_rgba8, d_linear_rgb, stream); });
}

int rvcp_render_frames_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *pushes, uint32_t n_frames,
                             uint32_t width, uint32_t height, uint32_t shard_index,
                             uint32_t shard_count, void *d_rgba8, void *d_linear_rgb, void *stream)
{
    return barrier(ctx, [&] {
        return impl_render_frames_async(ctx, pushes, n_frames, width, height, shard_index,
                                        shard_count, d_rgba8, d_linear_rgb, stream);
    });
}

int rvcp_render_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                      uint32_t height, void *d_rgba8, void *d_linear_rgb, void *stream)
{
    return barrier(ctx, [&] { return impl_render_async(ctx, push, width, height, d_rgba8,
        d_linear_rgb, stream); });
}

int rvcp_wait(rvcp_ctx_t *ctx, rvcp_stats_t *stats)
{
    return barrier(ctx, [&] { return impl_wait(ctx, stats); });
}

int rvcp_sync_stats(rvcp_ctx_t *ctx, rvcp_stats_t *stats)
{
    return barrier(ctx, [&] { return impl_sync_stats(ctx, stats); });
}

int rvcp_render(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                uint32_t height, uint8_t *out_rgba8, float *out_linear_rgb, rvcp_stats_t *stats)
{
    return barrier(ctx, [&] { return impl_render(ctx, push, width, height, out_rgba8,
        out_linear_rgb, stats); });
}

int rvcp_mandelbrot(rvcp_ctx_t *ctx, const rvcp_mandelbrot_push_t *push, uint32_t width,
                    uint32_t height, uint8_t *out_rgba8, float *out_value, rvcp_stats_t *stats)
{
    return barrier(ctx, [&] { return impl_mandelbrot(ctx, push, width, height, out_rgba8,
        out_value, stats); });
}

int rvcp_render_gbuffer_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                              uint32_t height, void *d_gbuffer, void *stream)
{
    return barrier(ctx, [&] { return impl_render_gbuffer_async(ctx, push, width, height, d_gbuffer, stream); });
}

int rvcp_denoise_params_default(rvcp_denoise_params_t *params)
{
    return barrier(nullptr, [&] { return impl_denoise_params_default(params); });
}

int rvcp_denoise_async(rvcp_ctx_t *ctx, const void *d_linear_rgb_in, const void *d_gbuffer,
                       uint32_t width, uint32_t height, const rvcp_denoise_params_t *params,
                       void *d_linear_rgb_out, void *d_rgba8_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_denoise_async(ctx, d_linear_rgb_in, d_gbuffer, width, height, params,
                                  d_linear_rgb_out, d_rgba8_out, stream);
    });
}

int rvcp_denoise_wait(rvcp_ctx_t *ctx, float *denoise_ms)
{
    return barrier(ctx, [&] { return impl_denoise_wait(ctx, denoise_ms); });
}

int rvcp_trace_rays_async(rvcp_ctx_t *ctx, const void *d_rays, uint32_t n_rays, uint32_t mode,
                          void *d_out, void *stream)
{
    return barrier(ctx, [&] { return impl_trace_rays_async(ctx, d_rays, n_rays, mode, d_out, stream); });
}

int rvcp_rays_wait(rvcp_ctx_t *ctx, float *rays_ms)
{
    return barrier(ctx, [&] { return impl_rays_wait(ctx, rays_ms); });
}

int rvcp_trace_rays(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, uint32_t n_rays, uint32_t mode,
                    void *out, float *rays_ms)
{
    return barrier(ctx, [&] { return impl_trace_rays(ctx, rays, n_rays, mode, out, rays_ms); });
}

int rvcp_primary_rays_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                            uint32_t height, void *d_rays, void *stream)
{
    return barrier(ctx, [&] { return impl_primary_rays_async(ctx, push, width, height, d_rays, stream); });
}

int rvcp_pick(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width, uint32_t height,
              uint32_t x, uint32_t y, rvcp_ray_hit_t *out_hit)
{
    return barrier(ctx, [&] { return impl_pick(ctx, push, width, height, x, y, out_hit); });
}

int rvcp_trace_paths_async(rvcp_ctx_t *ctx, const void *d_rays, const void *d_seeds,
                           uint32_t n_rays, uint32_t spp, void *d_linear_rgb_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_trace_paths_async(ctx, d_rays, d_seeds, n_rays, spp, d_linear_rgb_out, stream);
    });
}

int rvcp_paths_wait(rvcp_ctx_t *ctx, float *paths_ms, uint64_t *traversals)
{
    return barrier(ctx, [&] { return impl_paths_wait(ctx, paths_ms, traversals); });
}

int rvcp_trace_paths(rvcp_ctx_t *ctx, const rvcp_ray_t *rays, const float *seeds, uint32_t n_rays,
                     uint32_t spp, float *out_linear_rgb, float *paths_ms, uint64_t *traversals)
{
    return barrier(ctx, [&] {
        return impl_trace_paths(ctx, rays, seeds, n_rays, spp, out_linear_rgb, paths_ms, traversals);
    });
}

int rvcp_primary_seeds_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                             uint32_t height, void *d_seeds, void *stream)
{
    return barrier(ctx, [&] { return impl_primary_seeds_async(ctx, push, width, height, d_seeds, stream); });
}

int rvcp_render_denoised(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                         uint32_t height, const rvcp_denoise_params_t *params, uint8_t *out_rgba8,
                         float *out_linear_rgb, rvcp_stats_t *stats, float *denoise_ms)
{
    return barrier(ctx, [&] {
        return impl_render_denoised(ctx, push, width, height, params, out_rgba8, out_linear_rgb,
                                    stats, denoise_ms);
    });
}

int rvcp_temporal_params_default(rvcp_temporal_params_t *params)
{
    return barrier(nullptr, [&] { return impl_temporal_params_default(params); });
}

int rvcp_temporal_view_from_push(const rvcp_push_constant_t *push, uint32_t width, uint32_t height,
                                 rvcp_temporal_view_t *out_view)
{
    return barrier(nullptr, [&] { return impl_temporal_view_from_push(push, width, height, out_view); });
}

int rvcp_temporal_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                                   const void *d_cur_linear, const void *d_cur_gbuffer,
                                   const void *d_prev_linear, const void *d_prev_gbuffer,
                                   const void *d_prev_len, uint32_t width, uint32_t height,
                                   const rvcp_temporal_params_t *params, void *d_out_linear,
                                   void *d_out_len, void *d_rgba8_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_temporal_accumulate_async(ctx, view, d_cur_linear, d_cur_gbuffer, d_prev_linear,
                                              d_prev_gbuffer, d_prev_len, width, height, params,
                                              d_out_linear, d_out_len, d_rgba8_out, stream);
    });
}

int rvcp_temporal_wait(rvcp_ctx_t *ctx, float *temporal_ms)
{
    return barrier(ctx, [&] { return impl_temporal_wait(ctx, temporal_ms); });
}

int rvcp_temporal_reset(rvcp_ctx_t *ctx)
{
    return barrier(ctx, [&] { return impl_temporal_reset(ctx); });
}

int rvcp_render_temporal(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                         uint32_t height, const rvcp_temporal_params_t *tparams, uint32_t flags,
                         const rvcp_denoise_params_t *dparams, uint8_t *out_rgba8,
                         float *out_linear_rgb, uint32_t *out_history_len, rvcp_stats_t *stats,
                         float *temporal_ms, float *denoise_ms)
{
    return barrier(ctx, [&] {
        return impl_render_temporal(ctx, push, width, height, tparams, flags, dparams, out_rgba8,
                                    out_linear_rgb, out_history_len, stats, temporal_ms, denoise_ms);
    });
}

int rvcp_assemble_frame_async(rvcp_ctx_t *ctx, const void *d_gathered, uint32_t slot_rows,
                              uint32_t width, uint32_t height, uint32_t shard_count,
                              void *d_frame, void *stream)
{
    return barrier(ctx, [&] { return impl_assemble_frame_async(ctx, d_gathered, slot_rows,
        width, height, shard_count, d_frame, stream); });
}

int rvcp_rccl_unique_id(uint8_t *out_id)
{
    return barrier(nullptr, [&] { return impl_rccl_unique_id(out_id); });
}

int rvcp_rccl_init(rvcp_ctx_t *ctx, const uint8_t *id, uint32_t world, uint32_t rank)
{
    return barrier(ctx, [&] { return impl_rccl_init(ctx, id, world, rank); });
}

int rvcp_rccl_set_timeout(rvcp_ctx_t *ctx, uint32_t timeout_ms)
{
    return barrier(ctx, [&] { return impl_rccl_set_timeout(ctx, timeout_ms); });
}

int rvcp_rccl_attach(rvcp_ctx_t *ctx, void *nccl_comm, uint32_t world, uint32_t rank)
{
    return barrier(ctx, [&] { return impl_rccl_attach(ctx, nccl_comm, world, rank); });
}

int rvcp_gather_frame_async(rvcp_ctx_t *ctx, const void *d_shard_rgba8, uint32_t width,
                            uint32_t height, void *d_gathered, void *d_frame, void *stream)
{
    return barrier(ctx, [&] { return impl_gather_frame_async(ctx, d_shard_rgba8, width, height,
        d_gathered, d_frame, stream); });
}

int rvcp_gather_wait(rvcp_ctx_t *ctx, float *gather_ms, float *frame_ms)
{
    return barrier(ctx, [&] { return impl_gather_wait(ctx, gather_ms, frame_ms); });
}

int rvcp_svgf_params_default(rvcp_svgf_params_t *params)
{
    return barrier(nullptr, [&] { return impl_svgf_params_default(params); });
}

int rvcp_svgf_accumulate_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *view,
                               const void *d_cur_linear, const void *d_cur_gbuffer,
                               const void *d_prev_linear, const void *d_prev_gbuffer,
                               const void *d_prev_len, const void *d_prev_moments,
                               uint32_t width, uint32_t height,
                               const rvcp_temporal_params_t *tparams,
                               const rvcp_svgf_params_t *sparams, void *d_out_linear,
                               void *d_out_len, void *d_out_moments, void *d_rgba8_out,
                               void *stream)
{
    return barrier(ctx, [&] {
        return impl_svgf_accumulate_async(ctx, view, d_cur_linear, d_cur_gbuffer, d_prev_linear,
                                          d_prev_gbuffer, d_prev_len, d_prev_moments, width, height,
                                          tparams, sparams, d_out_linear, d_out_len, d_out_moments,
                                          d_rgba8_out, stream);
    });
}

int rvcp_svgf_filter_async(rvcp_ctx_t *ctx, const void *d_linear, const void *d_moments,
                           const void *d_len, const void *d_gbuffer, uint32_t width,
                           uint32_t height, const rvcp_svgf_params_t *params,
                           void *d_linear_out, void *d_variance_out, void *d_feedback_out,
                           void *d_rgba8_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_svgf_filter_async(ctx, d_linear, d_moments, d_len, d_gbuffer, width, height,
                                      params, d_linear_out, d_variance_out, d_feedback_out,
                                      d_rgba8_out, stream);
    });
}

int rvcp_svgf_wait(rvcp_ctx_t *ctx, float *accumulate_ms, float *filter_ms)
{
    return barrier(ctx, [&] { return impl_svgf_wait(ctx, accumulate_ms, filter_ms); });
}

int rvcp_render_svgf(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                     uint32_t height, const rvcp_temporal_params_t *tparams,
                     const rvcp_svgf_params_t *sparams, uint32_t flags, uint8_t *out_rgba8,
                     float *out_linear_rgb, float *out_variance, uint32_t *out_history_len,
                     rvcp_stats_t *stats, float *accumulate_ms, float *filter_ms)
{
    return barrier(ctx, [&] {
        return impl_render_svgf(ctx, push, width, height, tparams, sparams, flags, out_rgba8,
                                out_linear_rgb, out_variance, out_history_len, stats,
                                accumulate_ms, filter_ms);
    });
}

int rvcp_svgf_reset(rvcp_ctx_t *ctx)
{
    return barrier(ctx, [&] { return impl_svgf_reset(ctx); });
}

int rvcp_demodulate_async(rvcp_ctx_t *ctx, const void *d_linear, const void *d_gbuffer,
                          uint32_t width, uint32_t height, void *d_irradiance_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_demodulate_async(ctx, d_linear, d_gbuffer, width, height, d_irradiance_out,
                                     stream);
    });
}

int rvcp_remodulate_async(rvcp_ctx_t *ctx, const void *d_irradiance, const void *d_gbuffer,
                          uint32_t width, uint32_t height, void *d_linear_out, void *d_rgba8_out,
                          void *stream)
{
    return barrier(ctx, [&] {
        return impl_remodulate_async(ctx, d_irradiance, d_gbuffer, width, height, d_linear_out,
                                     d_rgba8_out, stream);
    });
}

int rvcp_albedo_wait(rvcp_ctx_t *ctx, float *demodulate_ms, float *remodulate_ms)
{
    return barrier(ctx, [&] { return impl_albedo_wait(ctx, demodulate_ms, remodulate_ms); });
}

int rvcp_set_demodulation(rvcp_ctx_t *ctx, int on)
{
    return barrier(ctx, [&] { return impl_set_demodulation(ctx, on); });
}

int rvcp_get_demodulation(rvcp_ctx_t *ctx, int *on)
{
    return barrier(ctx, [&] { return impl_get_demodulation(ctx, on); });
}

int rvcp_taa_jitter(uint32_t frame_index, float out_jitter[2])
{
    return barrier(nullptr, [&] { return impl_taa_jitter(frame_index, out_jitter); });
}

int rvcp_taa_jitter_push(const rvcp_push_constant_t *base, uint32_t width, uint32_t height,
                         const float jitter[2], rvcp_push_constant_t *out)
{
    return barrier(nullptr, [&] { return impl_taa_jitter_push(base, width, height, jitter, out); });
}

int rvcp_taa_params_default(rvcp_taa_params_t *params)
{
    return barrier(nullptr, [&] { return impl_taa_params_default(params); });
}

int rvcp_taa_resolve_async(rvcp_ctx_t *ctx, const rvcp_temporal_view_t *cur_view,
                           const rvcp_temporal_view_t *prev_view, const void *d_cur_linear,
                           const void *d_cur_gbuffer, const void *d_prev_resolved,
                           const void *d_prev_len, uint32_t width, uint32_t height,
                           const rvcp_taa_params_t *params, void *d_out_resolved,
                           void *d_out_len, void *d_rgba8_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_taa_resolve_async(ctx, cur_view, prev_view, d_cur_linear, d_cur_gbuffer,
                                      d_prev_resolved, d_prev_len, width, height, params,
                                      d_out_resolved, d_out_len, d_rgba8_out, stream);
    });
}

int rvcp_taa_wait(rvcp_ctx_t *ctx, float *taa_ms)
{
    return barrier(ctx, [&] { return impl_taa_wait(ctx, taa_ms); });
}

int rvcp_set_taa(rvcp_ctx_t *ctx, int on)
{
    return barrier(ctx, [&] { return impl_set_taa(ctx, on); });
}

int rvcp_get_taa(rvcp_ctx_t *ctx, int *on)
{
    return barrier(ctx, [&] { return impl_get_taa(ctx, on); });
}

int rvcp_taa_reset(rvcp_ctx_t *ctx)
{
    return barrier(ctx, [&] { return impl_taa_reset(ctx); });
}

int rvcp_taau_params_default(rvcp_taau_params_t *params)
{
    return barrier(nullptr, [&] { return impl_taau_params_default(params); });
}

int rvcp_taa_upsample_async(rvcp_ctx_t *ctx, uint32_t scale, const rvcp_temporal_view_t *jit_view,
                            const rvcp_temporal_view_t *cur_view,
                            const rvcp_temporal_view_t *prev_view, const void *d_cur_linear,
                            const void *d_gbuffer_hi, const void *d_prev_resolved,
                            const void *d_prev_weight, uint32_t width, uint32_t height,
                            const rvcp_taau_params_t *params, void *d_out_resolved,
                            void *d_out_weight, void *d_rgba8_out, void *stream)
{
    return barrier(ctx, [&] {
        return impl_taa_upsample_async(ctx, scale, jit_view, cur_view, prev_view, d_cur_linear,
                                       d_gbuffer_hi, d_prev_resolved, d_prev_weight, width, height,
                                       params, d_out_resolved, d_out_weight, d_rgba8_out, stream);
    });
}

int rvcp_taau_wait(rvcp_ctx_t *ctx, float *taau_ms)
{
    return barrier(ctx, [&] { return impl_taau_wait(ctx, taau_ms); });
}

int rvcp_set_taa_upsample(rvcp_ctx_t *ctx, uint32_t scale)
{
    return barrier(ctx, [&] { return impl_set_taa_upsample(ctx, scale); });
}

int rvcp_get_taa_upsample(rvcp_ctx_t *ctx, uint32_t *scale)
{
    return barrier(ctx, [&] { return impl_get_taa_upsample(ctx, scale); });
}

int rvcp_set_sampling(rvcp_ctx_t *ctx, int32_t sampling)
{
    return barrier(ctx, [&] { return impl_set_sampling(ctx, sampling); });
}

int rvcp_get_sampling(rvcp_ctx_t *ctx, int32_t *sampling)
{
    return barrier(ctx, [&] { return impl_get_sampling(ctx, sampling); });
}

int rvcp_set_materials(rvcp_ctx_t *ctx, int32_t materials)
{
    return barrier(ctx, [&] { return impl_set_materials(ctx, materials); });
}

int rvcp_get_materials(rvcp_ctx_t *ctx, int32_t *materials)
{
    return barrier(ctx, [&] { return impl_get_materials(ctx, materials); });
}

int rvcp_render_spp_map_async(rvcp_ctx_t *ctx, const rvcp_push_constant_t *push, uint32_t width,
                              uint32_t height, const void *d_spp_map, uint32_t spp_hint,
                              void *d_rgba8, void *d_linear_rgb, void *stream)
{
    return barrier(ctx, [&] { return impl_render_spp_map_async(ctx, push, width, height, d_spp_map,
        spp_hint, d_rgba8, d_linear_rgb, stream); });
}

int rvcp_adaptive_params_default(rvcp_adaptive_params_t *params)
{
    return barrier(nullptr, [&] { return impl_adaptive_params_default(params); });
}

int rvcp_spp_plan_async(rvcp_ctx_t *ctx, const void *d_variance, const void *d_linear,
                        const void *d_len, const void *d_gbuffer, uint32_t width, uint32_t height,
                        const rvcp_adaptive_params_t *params, void *d_spp_map_out, void *stream)
{
    return barrier(ctx, [&] { return impl_spp_plan_async(ctx, d_variance, d_linear, d_len, d_gbuffer,
        width, height, params, d_spp_map_out, stream); });
}

int rvcp_spp_plan_wait(rvcp_ctx_t *ctx, float *plan_ms, uint64_t *planned_samples)
{
    return barrier(ctx, [&] { return impl_spp_plan_wait(ctx, plan_ms, planned_samples); });
}

int rvcp_set_adaptive(rvcp_ctx_t *ctx, const rvcp_adaptive_params_t *params)
{
    return barrier(ctx, [&] { return impl_set_adaptive(ctx, params); });
}

int rvcp_get_adaptive(rvcp_ctx_t *ctx, int *on, rvcp_adaptive_params_t *out_params)
{
    return barrier(ctx, [&] { return impl_get_adaptive(ctx, on, out_params); });
}

int rvcp_adaptive_last_map(rvcp_ctx_t *ctx, uint32_t *out_map, uint32_t *out_width,
                           uint32_t *out_height)
{
    return barrier(ctx, [&] { return impl_adaptive_last_map(ctx, out_map, out_width, out_height); });
}

}  // extern "C"
