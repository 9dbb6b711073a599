// rvcp_kernels_map.hip -- the pre-pass family with a per-pixel sample count
// (rvcp_render_spp_map_async): rvcp_kernels.hip compiled with RVCP_SPP_MAP = 1.
// That file then holds only the primary kernels, the path kernels of schedules 3, 4, 5, 6 and
// 10 and the BVH path kernel, as games101_map_*, and their launcher and occupancy query behind the
// KernelBuild rvcp_games101_map_build (kKernelBuilds[0][1], rvcp_internal.h).  A translation unit
// of its own, so that the default kernels are compiled from a text that does not mention the map.
#define RVCP_SPP_MAP 1
#include "rvcp_kernels.hip"
