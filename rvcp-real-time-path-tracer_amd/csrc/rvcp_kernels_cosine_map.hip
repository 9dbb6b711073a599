// rvcp_kernels_cosine_map.hip -- the map build (rvcp_kernels_map.hip) of the cosine-weighted
// bounce (RVCP_SAMPLING_COSINE): rvcp_kernels.hip compiled with
// RVCP_SAMPLING = 1 and RVCP_SPP_MAP = 1, its kernels as games101_cosine_map_*, its launcher and
// occupancy query behind the KernelBuild rvcp_games101_cosine_map_build (kKernelBuilds[1][1]).
#define RVCP_SAMPLING 1
#define RVCP_SPP_MAP 1
#include "rvcp_kernels.hip"
