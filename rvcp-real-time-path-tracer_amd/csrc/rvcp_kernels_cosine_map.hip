// rvcp_kernels_cosine_map.hip -- the map build (rvcp_kernels_map.hip) of the cosine-weighted
// bounce (RVCP_SAMPLING_COSINE): rvcp_kernels.hip compiled with
// RVCP_SAMPLING = 1 and RVCP_SPP_MAP = 1, its kernels as games101_cosine_map_*, its launcher and
// occupancy query as rvcp_launch_games101_v3_cosine_map and rvcp_games101_occupancy_cosine_map.
#define RVCP_SAMPLING 1
#define RVCP_SPP_MAP 1
#include "rvcp_kernels.hip"
