// rvcp_frame_plan.h -- what a render decides before it touches the device: the kernel schedule,
// which scene-specialised kernels replace the built-in ones, and the persistent grid
// (rvcp_frame_plan.cpp).  A pure function of plain numbers: no HIP, no context, so it is also
// built and checked on the CPU (tools/frame_plan_check.cpp, tests/test_frame_plan_cpu.py).
#pragma once

#include "../../include/rvcp.h"
#include "rvcp_internal.h"

namespace rvcp {

struct FramePlanIn {
    // rvcp_config_t
    int32_t integrator = RVCP_INTEGRATOR_GAMES101;
    int32_t kernel_variant = 0;
    int32_t accel = RVCP_ACCEL_NONE;
    uint32_t spp = 1, max_bounces = 0;
    float attenuation_stop_eps = 0.0f, ray_t_min = 0.0f;
    uint32_t grid_waves_per_simd = 0;
    // the scene
    uint32_t n_faces = 0;
    uint32_t bvh_prefix = 0;            // faces the BVH hybrid keeps out of the BVH
    // the device
    uint32_t n_simds = 0;
    // resident workgroups of the built-in kernels for the context's bounce sampling: per
    // schedule, of the BVH path kernel and of the mode-2 kernel
    int grid_capacity[kMaxVariant + 1] = {};
    int bvh_capacity = 0, legacy_capacity = 0;
    // the scene's specialised module (JitKernels), if any
    bool module = false;
    int blocks_per_cu5 = 0, blocks_per_cu6 = 0, blocks_per_cu_bvh = 0, blocks_per_cu_legacy = 0;
    bool has_legacy = false, has_bvh_path = false, has_bvh_primary = false;
    // the frames: this shard's pixels per frame and the pixels from one frame of a batch to the next
    uint32_t n_frames = 1, frame_px = 0, stride = 0;
    // debug build of the library: FrameArgs::spread_min (0 in the product)
    uint32_t spread_min = 0;
};

struct FramePlan {
    int status = RVCP_OK;               // or RVCP_E_UNSUPPORTED: a batch on schedule 1 or 2
    int32_t variant = 0;                // FrameArgs::variant, FrameArgs::accel
    int32_t accel = RVCP_ACCEL_NONE;
    bool trivial = false;               // every sample is black before its first traversal
    bool legacy = false;                // integrator mode 2
    // the module's kernels replace: the schedule-3/6 pre-pass and path kernel, the BVH ones,
    // the mode-2 kernel
    bool spec = false, spec_bvh = false, spec_legacy = false;
    bool cams = false;                  // the batch needs its FrameCam records on the device
    bool prepass_batched = false;       // ... and its pre-passes run as one launch
    uint32_t out_px = 0;                // pixels the outputs span: a batch's frames lie `stride` apart
    // the persistent grid of a frame that launches a path kernel (0 for a trivial or empty one)
    uint32_t cap = 0;                   // resident workgroups, after the caller's limit
    uint32_t wpb = 0;                   // waves per workgroup
    uint32_t blocks = 0;
    uint32_t static_chunk = 0, static_chunks = 0;
    int32_t stats_code = 0;             // rvcp_stats_t::kernel_variant
};

FramePlan plan_frame(const FramePlanIn &in);

// FrameArgs::accel: the BVH is traversed only where the scene has faces
inline int32_t resolved_accel(int32_t cfg_accel, uint32_t n_faces)
{
    return (cfg_accel == RVCP_ACCEL_BVH && n_faces > 0) ? RVCP_ACCEL_BVH : RVCP_ACCEL_NONE;
}

}  // namespace rvcp
