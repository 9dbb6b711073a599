// rvcp_frame_plan.cpp -- the schedule, specialisation and grid decision of a render
// (rvcp_frame_plan.h).  No HIP: the library builds it with hipcc, the CPU check with g++.
#include "rvcp_frame_plan.h"

namespace rvcp {

FramePlan plan_frame(const FramePlanIn &in)
{
    FramePlan P;
    const uint64_t frame_samples = (uint64_t)in.frame_px * in.spp;
    // automatic schedule: 10 / 5 (LDS tiles; the workgroup's rays pooled into full passes on
    // large frames, one ray per lane on small ones) for large meshes, 10 also for mid-size
    // meshes on large frames, else 3, or 6 (6 waves/SIMD) for
    // large frames -- with the scene-specialised scan only for very large frames
    // (kSpecWideMinSamples: its 6-wave build is slower below)
    const bool jit_ok = in.module && in.ray_t_min > 0.0f;
    const bool big_frame = frame_samples >= kTiledDualMinSamples;
    P.variant = in.kernel_variant != 0 ? in.kernel_variant
              : in.n_faces >= kTiledMinFaces ? (big_frame ? kTiledPoolVariant : 5)
              : (!jit_ok && in.n_faces > kTiledWideMinFaces && big_frame) ? kTiledPoolVariant
              : (frame_samples >= (jit_ok ? kSpecWideMinSamples : kWideMinSamples)) ? 6
              : kDefaultVariant;
    P.accel = resolved_accel(in.accel, in.n_faces);
    if (P.accel == RVCP_ACCEL_BVH) P.variant = 3;    // the BVH traversal lives in the v3 kernels
    const uint32_t bvh_prefix = P.accel == RVCP_ACCEL_BVH ? in.bvh_prefix : 0u;
    P.legacy = in.integrator == RVCP_INTEGRATOR_LEGACY;

    // With MAX_BOUNCES == 0 or ATTENUATION_STOP_EPS > 1 every sample returns 0 before its
    // first traversal (:413-419): the frame is black.  ray_tracer.comp has no attenuation
    // test before its first traversal (:629-634).
    P.trivial = in.max_bounces == 0 || (!P.legacy && 1.0f < in.attenuation_stop_eps);
    // a batch shares one surface list and one path kernel: the pre-pass schedules (3-6, 10 and
    // the persistent BVH path kernel) only
    if (in.n_frames > 1 && !P.trivial && !P.legacy && P.variant < 3) {
        P.status = RVCP_E_UNSUPPORTED;
        return P;
    }
    // a batch's cameras and times in device memory: mode 2's one kernel and the pre-pass
    // schedules' one pre-pass launch read them per frame
    P.cams = in.n_frames > 1 && !P.trivial && in.frame_px > 0 && (P.legacy || P.variant >= 3);
    P.prepass_batched = P.cams && in.frame_px <= kPrepassBatchMaxPixels;
    P.out_px = in.n_frames > 1 ? in.n_frames * in.stride : in.frame_px;
    if (P.trivial || in.frame_px == 0) return P;     // a fill, or nothing: stats code 0

    // the scene-specialised path kernel (§4.7) replaces schedules 3 and 6 when the
    // upload compiled one; its exactness argument needs t_min > 0
    const int jit_per_cu = !in.module ? 0 : P.variant == 6 ? in.blocks_per_cu6
                         : P.variant == 3 ? in.blocks_per_cu5 : 0;
    P.spec = !P.legacy && !P.accel && jit_per_cu > 0 && in.ray_t_min > 0.0f;
    // mode 2 with the specialised triangle scan (its kernel also checks per wave
    // that every ray is finite and has t_min > 0)
    P.spec_legacy = P.legacy && in.module && in.has_legacy && in.blocks_per_cu_legacy > 0;
    // the BVH hybrid's kernels (the prefix faces by the specialised scan); without them
    // (t_min <= 0) the built-in BVH kernels test the prefix with the generic test
    P.spec_bvh = !P.legacy && P.accel && bvh_prefix > 0 && in.module && in.has_bvh_path &&
                 in.has_bvh_primary && in.blocks_per_cu_bvh > 0 && in.ray_t_min > 0.0f;
    uint32_t cap = (uint32_t)(P.legacy ? in.legacy_capacity
                             : P.accel ? in.bvh_capacity : in.grid_capacity[P.variant]);
    if (P.spec) cap = (uint32_t)jit_per_cu * (in.n_simds / 4u);
    if (P.spec_bvh) cap = (uint32_t)in.blocks_per_cu_bvh * (in.n_simds / 4u);
    if (P.spec_legacy) cap = (uint32_t)in.blocks_per_cu_legacy * (in.n_simds / 4u);
    P.wpb = (uint32_t)((P.legacy || P.accel ? kBlock : variant_block(P.variant)) / kWave);
    if (in.grid_waves_per_simd > 0) {     // the caller's grid per frame (rvcp.h)
        const uint64_t lim = (uint64_t)in.grid_waves_per_simd * in.n_simds / P.wpb;
        if (lim < cap) cap = lim > 0 ? (uint32_t)lim : 1u;
    }
    P.cap = cap;
    uint32_t waves = 0, chunk = 0;
    static_split(in.frame_px * in.n_frames, cap * P.wpb, in.n_simds, waves, chunk);   // the queue of the whole batch
    P.blocks = (waves + P.wpb - 1) / P.wpb;
    if (P.blocks > cap) P.blocks = cap;
    if (P.blocks == 0) P.blocks = 1;
    P.static_chunk = chunk;
    P.static_chunks = waves * chunk;
    // schedules 3/6 spreading a small surface list run the full resident grid
    if (in.spread_min && !P.legacy && !P.accel && (P.variant == 3 || P.variant == 6)) P.blocks = cap;

    P.stats_code = P.legacy ? 8 : P.accel ? 7 : P.variant;
    if (P.spec || P.spec_bvh || P.spec_legacy) P.stats_code |= RVCP_VARIANT_SPECIALIZED;
    return P;
}

}  // namespace rvcp
