// rvcp_jit.h -- scene-specialised path kernels compiled at upload with hipRTC (rvcp_jit.cpp,
// DESIGN.md §4.7).  Host-side only; not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rvcp.h"
#include "rvcp_internal.h"

namespace rvcp {

struct JitKernels {
    int device = 0;
    hipModule_t module = nullptr;
    hipFunction_t path5 = nullptr;     // schedule 3 (5 waves per SIMD)
    hipFunction_t path6 = nullptr;     // schedule 6 (6 waves per SIMD)
    hipFunction_t legacy = nullptr;    // integrator mode 2 (modules compiled with `legacy`)
    hipFunction_t primary = nullptr;   // the schedule-3/6 pre-pass with the specialised scan
    // the BVH hybrid (modules compiled with `bvh`): the BVH path kernel and pre-pass, the scan
    // covering the scene's first FrameArgs::bvh_prefix faces
    hipFunction_t bvh_path = nullptr, bvh_primary = nullptr;
    int blocks_per_cu5 = 0, blocks_per_cu6 = 0, blocks_per_cu_legacy = 0, blocks_per_cu_bvh = 0;
    // fnv1a of the module's whole compile input (hipRTC version, options, embedded sources,
    // generated scan): the disk-cache key, and the identity bench.py binds PMC summaries to
    uint64_t key_hash = 0;
    ~JitKernels();
};

// Every |v0| <= 2^40 and |e1|, |e2| <= 2^41 (finite): the range in which dropping the products
// with exact-zero components cannot turn the generic test's inf * 0 = NaN into a finite value.
bool jit_scene_in_range(const TriRecord *tri, uint32_t n);
// Every triangle's denominator, for any ray direction passing the kernel's dir_fast_ok (each
// component +-0 or at least 2^-40, |d|_1 <= 16), is +-0 or within [2^-126, 2^126] in magnitude
// with no overflow on the way: the generic scan may then take 1/den without the class check
// (FrameArgs::rcp_fast).
bool scan_rcp_fast_scene(const TriRecord *tri, uint32_t n);
// Extra hipRTC options (debug build only; empty in the product library).
std::vector<std::string> jit_extra_flags();
// The generated scan (spec_scan1 / spec_scan2) for n triangle records.
// opts: kScanSkipB | kScanEagerSplit (experiment knobs, jit_scan_opts)
constexpr unsigned kScanSkipB = 1u, kScanEagerSplit = 2u;
std::string jit_scan_source(const TriRecord *tri, uint32_t n, unsigned opts = 0);
// Face groups: the partition of a scene's faces into an always set and groups
// that a ray tests only when it reaches the group's padded box or runs nearly parallel to one of
// its planes.  lum_mask: bit i set for a luminous face i (they stay in the always set).
struct ScanGroup {
    std::vector<uint32_t> faces;                 // ascending
    float lo[3], hi[3];                          // the padded box, rounded outward
    std::vector<std::array<double, 3>> normals;  // one unit normal per distinct plane direction
};
struct ScanGroups {
    std::vector<int> group_of;                   // per face: its group, or -1 (always set)
    std::vector<ScanGroup> groups;
    float centre[3] = {0, 0, 0}, reach[3] = {0, 0, 0};   // origins admitted: |o - centre| <= reach
};
ScanGroups jit_scan_groups(const TriRecord *tri, uint32_t n, uint64_t lum_mask);
// The grouped scan's text (RVCP_SPEC_GROUPS, spec_group_origin_ok, spec_group_reach, spec_always1/2,
// spec_group_scan), appended to a games101 module's scan; "" for a scene without an eligible group.
std::string jit_groups_source(const TriRecord *tri, uint32_t n, uint64_t lum_mask, unsigned opts = 0);
// What a module is compiled with besides its scan: the options' variant defines (jit_options)
// and so, with the scan, the module's compile key.
struct JitCompile {
    bool legacy = false;        // also the mode-2 kernel (RVCP_JIT_LEGACY) ...
    int legacy_waves = 0;       // ... for this many waves per SIMD (0: the compiler's choice)
    bool lds_scene = false;     // ... which copies the scene into LDS (RVCP_LEGACY_LDS_SCENE)
    bool bvh = false;           // also the BVH hybrid's kernels (RVCP_JIT_BVH)
    int sampling = RVCP_SAMPLING_UNIFORM;   // -DRVCP_SAMPLING (none for the default)
    bool spp_map = false;       // -DRVCP_SPP_MAP=1
};
// Compile rvcp_kernels.hip with the given scan for gfx950 (hipRTC); 0 or -1 with err set.
int jit_compile_code(const std::string &scan, std::vector<char> &code, std::string &err,
                     const JitCompile &cc);
// jit_compile_code behind the on-disk code-object cache (rvcp_set_code_cache_dir): a verified
// entry for exactly this compile is read (*from_disk = true), else the module is compiled and
// stored; force_compile counts the entry rejected and recompiles it (the runtime refused it).
int jit_cached_code(const std::string &scan, std::vector<char> &code, std::string &err,
                    const JitCompile &cc, bool *from_disk, bool force_compile);
// Which module a scene gets.
struct JitSpec {
    bool legacy = false;        // the module also holds the mode-2 kernel
    // (legacy) no spheres: the mode-2 kernel is built for 6 waves per SIMD
    bool sphereless = false;
    // (legacy) at most 64 spheres and 64 materials (and, as always here, 64 faces): the mode-2
    // kernel reads its hit records, spheres and materials from LDS copies
    bool lds_fits = false;
    bool bvh = false;           // also the BVH hybrid's kernels; tri / n are then the prefix faces
    // the bounce the module's games101 kernels are compiled with (RVCP_SAMPLING_*, DESIGN.md
    // §4.17); part of the module's source tag and of its compile key
    int sampling = RVCP_SAMPLING_UNIFORM;
    // the module's pre-pass family takes a per-pixel sample count (DESIGN.md §4.18:
    // rvcp_spec_primary_kernel and rvcp_spec_bvh_primary_kernel then have one more parameter, the
    // map); part of the source tag and of the compile key likewise
    bool spp_map = false;
    // (legacy) the scene's sphere records, written into the module as literals
    // (jit_sphere_source) -- the module is then valid for these spheres only, like its scan
    const rvcp_sphere_t *spheres = nullptr;
    uint32_t n_spheres = 0, n_materials = 64;
    // the scene's luminous faces (bit i: face i), which the grouped scan keeps in its always set;
    // read only for a module that may get face groups (neither legacy nor bvh)
    uint64_t lum_mask = 0;
};
// Compiled + loaded kernels for the scene on `device` (process-wide cache keyed by the module's
// source text: the scan and the spec's tags); nullptr with err set when hipRTC is unavailable or
// compilation fails.
std::shared_ptr<JitKernels> jit_path_kernels(int device, const TriRecord *tri, uint32_t n,
                                             const JitSpec &spec, std::string &err);
// The sphere X-macro of a mode-2 module ("" for none or more than kJitMaxSpheres).
constexpr uint32_t kJitMaxSpheres = 64;
std::string jit_sphere_source(const rvcp_sphere_t *sph, uint32_t n);
// The LDS sizes of a mode-2 module with the scene in LDS, and its LDS primary-hit columns.
std::string jit_legacy_lds_source(uint32_t n_faces, uint32_t n_spheres, uint32_t n_materials);

}  // namespace rvcp
