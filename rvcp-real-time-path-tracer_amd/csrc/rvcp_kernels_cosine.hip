// rvcp_kernels_cosine.hip -- the games101 kernels with the cosine-weighted bounce
// (RVCP_SAMPLING_COSINE): rvcp_kernels.hip compiled with RVCP_SAMPLING = 1.
// That file then holds only the games101 kernels (every schedule, the BVH path kernel) as
// games101_cosine_*, and their launchers and occupancy query behind the KernelBuild
// rvcp_games101_cosine_build (kKernelBuilds[1][0], rvcp_internal.h); the pre-pass is the same
// template as the default object's.  A translation unit of its own, so that the default
// kernels are compiled from a text that does not mention the mode.
#define RVCP_SAMPLING 1
#include "rvcp_kernels.hip"
