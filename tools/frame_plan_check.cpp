// frame_plan_check.cpp -- CPU driver of librvcp's frame plan (csrc/rvcp_frame_plan.cpp: the
// schedule, specialisation and grid decision of a render), built with g++ under
// AddressSanitizer / UBSan by tests/test_frame_plan_cpu.py from that file alone.
// Reads one plan input per line from stdin, the fields of FramePlanIn in declaration order
// (tests/frame_plan_ref.py FIELDS), and prints the plan of each, one line per input:
//   status variant accel trivial legacy spec spec_bvh spec_legacy cams prepass_batched out_px
//   cap wpb blocks static_chunk static_chunks stats_code
// "split N GRID_WAVES N_SIMDS" lines print static_split's "waves chunk" instead.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rvcp_frame_plan.h"

int main()
{
    char line[1024];
    while (std::fgets(line, sizeof(line), stdin)) {
        uint32_t n = 0, grid_waves = 0, n_simds = 0;
        if (std::sscanf(line, "split %" SCNu32 " %" SCNu32 " %" SCNu32, &n, &grid_waves, &n_simds) == 3) {
            uint32_t waves = 0, chunk = 0;
            rvcp::static_split(n, grid_waves, n_simds, waves, chunk);
            std::printf("%" PRIu32 " %" PRIu32 "\n", waves, chunk);
            continue;
        }
        rvcp::FramePlanIn in;
        int *c = in.grid_capacity;
        int module = 0, has_legacy = 0, has_bvh_path = 0, has_bvh_primary = 0;
        static_assert(rvcp::kMaxVariant == 10, "eleven capacities per line");
        const int got = std::sscanf(
            line,
            "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNu32 " %" SCNu32 " %f %f %" SCNu32
            " %" SCNu32 " %" SCNu32 " %" SCNu32 " %d %d %d %d %d %d %d %d %d %d %d %d %d"
            " %d %d %d %d %d %d %d %d %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32,
            &in.integrator, &in.kernel_variant, &in.accel, &in.spp, &in.max_bounces,
            &in.attenuation_stop_eps, &in.ray_t_min, &in.grid_waves_per_simd, &in.n_faces,
            &in.bvh_prefix, &in.n_simds, c, c + 1, c + 2, c + 3, c + 4, c + 5, c + 6, c + 7, c + 8,
            c + 9, c + 10, &in.bvh_capacity, &in.legacy_capacity, &module, &in.blocks_per_cu5,
            &in.blocks_per_cu6, &in.blocks_per_cu_bvh, &in.blocks_per_cu_legacy, &has_legacy,
            &has_bvh_path, &has_bvh_primary, &in.n_frames, &in.frame_px, &in.stride, &in.spread_min);
        if (got != 36) {
            std::fprintf(stderr, "frame_plan_check: %d of 36 fields in: %s", got, line);
            return 2;
        }
        in.module = module != 0;
        in.has_legacy = has_legacy != 0;
        in.has_bvh_path = has_bvh_path != 0;
        in.has_bvh_primary = has_bvh_primary != 0;
        const rvcp::FramePlan P = rvcp::plan_frame(in);
        std::printf("%d %d %d %d %d %d %d %d %d %d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32
                    " %" PRIu32 " %" PRIu32 " %d\n",
                    P.status, P.variant, P.accel, (int)P.trivial, (int)P.legacy, (int)P.spec,
                    (int)P.spec_bvh, (int)P.spec_legacy, (int)P.cams, (int)P.prepass_batched,
                    P.out_px, P.cap, P.wpb, P.blocks, P.static_chunk, P.static_chunks, P.stats_code);
    }
    return 0;
}
