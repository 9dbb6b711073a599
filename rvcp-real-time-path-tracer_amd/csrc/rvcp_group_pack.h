// rvcp_group_pack.h -- how the items of the grouped scan are laid out over its passes
// (spec_group_pass, rvcp_kernels.hip; DESIGN.md §4.7 "Face groups").  Plain C++, host and device,
// no HIP types: tests/test_group_pack_cpu.py compiles it with g++.
//
// A wave holds c[g] items of group g (slot A's, then slot B's), G <= 4 groups, c[g] <= 128.  Pass
// p scans the 64 items whose virtual index lies in [64 p, 64 p + 64), one per lane, one group
// after the other, so a pass costs one scan per group it holds.  In group order, with f the
// running fill: a group starts at f if its items then span no more passes than ceil(c / 64),
//     (f & 63) + ((c - 1) & 63) + 1 <= 64,
// and otherwise at f rounded up to the next multiple of 64.  Hence
//   * every group is scanned ceil(c / 64) times, the minimum;
//   * with 64 items or fewer in all there is one pass (no group straddles, so none is padded);
//   * padding only ever precedes a group's start: the occupied lanes of a pass are a prefix
//     (rvcp_group_pack_lanes), and each padding avoids exactly one straddle -- one scan -- for at
//     most one more pass, so the cost is never above the unpadded numbering's.
#pragma once
#ifndef __HIPCC_RTC__             // hipRTC provides the fixed-width types
#include <stdint.h>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define RVCP_GROUP_PACK_FN __host__ __device__ __forceinline__
#else
#define RVCP_GROUP_PACK_FN static inline
#endif

#define RVCP_GROUP_PACK_MAX_GROUPS 4
#define RVCP_GROUP_PACK_WIDTH 64u

// start[g]: the virtual index of group g's first item (an empty group gets the running fill and
// holds no index); returns the number of passes.
// (RVCP_GROUP_PACK_CONTIGUOUS: the unpadded numbering, for A/B measurements only.)
RVCP_GROUP_PACK_FN uint32_t rvcp_group_pack(const uint32_t *c, int n_groups, uint32_t *start) {
    uint32_t f = 0u;
    for (int g = 0; g < n_groups; g++) {
#ifndef RVCP_GROUP_PACK_CONTIGUOUS
        if (c[g] != 0u && (f & 63u) + ((c[g] - 1u) & 63u) + 1u > RVCP_GROUP_PACK_WIDTH)
            f = (f + 63u) & ~63u;
#endif
        start[g] = f;
        f += c[g];
    }
    return (f + 63u) >> 6;
}

// Does group g hold an item of pass p?
RVCP_GROUP_PACK_FN bool rvcp_group_pack_in_pass(uint32_t c_g, uint32_t start_g, uint32_t p) {
    return c_g != 0u && start_g < 64u * p + 64u && start_g + c_g > 64u * p;
}

// The lanes of pass p that group g's items occupy: [lo, hi) (call only if the group is in p).
RVCP_GROUP_PACK_FN void rvcp_group_pack_span(uint32_t c_g, uint32_t start_g, uint32_t p, uint32_t *lo,
                                             uint32_t *hi) {
    const uint32_t p0 = 64u * p, e = start_g + c_g;
    *lo = start_g > p0 ? start_g - p0 : 0u;
    *hi = e < p0 + 64u ? e - p0 : 64u;
}

// The number of occupied lanes of pass p: lanes [0, n) hold items, the rest none.
RVCP_GROUP_PACK_FN uint32_t rvcp_group_pack_lanes(const uint32_t *c, const uint32_t *start, int n_groups,
                                                  uint32_t p) {
    uint32_t n = 0u;
    for (int g = 0; g < n_groups; g++)
        if (rvcp_group_pack_in_pass(c[g], start[g], p)) {
            uint32_t lo, hi;
            rvcp_group_pack_span(c[g], start[g], p, &lo, &hi);
            if (hi > n) n = hi;
        }
    return n;
}

// The virtual index of an item: slot A's items of a group first, in rank order, then slot B's.
RVCP_GROUP_PACK_FN uint32_t rvcp_group_pack_item(uint32_t start_g, uint32_t n_a, int slot_b, uint32_t rank) {
    return start_g + (slot_b ? n_a : 0u) + rank;
}
