"""Shared by the face-group tests (tests/test_jit_groups_cpu.py, tests/test_gpu_spec_groups.py;
DESIGN.md §4.7 "Face groups"): the scenes, and the CPU build of the generated grouped scan next to
the ungrouped one and a reference loop.

The CPU build compiles rvcp_jit.cpp's text with g++ (tests/test_jit_cpu.py's prelude) and drives it
as the kernel's spec_group_pass does for one ray: the always-set scan, the reach test with that
bound, every reached group's scan started from that same bound, the results merged by the
order-free rule (smaller t, or equal t and larger face; the shadow slot keeps t alone).  The reach
test's slab reciprocal is the IEEE quotient moved by `rcp_mode` ulps (-1, 0, +1): the device's
v_rcp_f32 is within 1 ulp of it.  Pure test infrastructure."""
import ctypes
import subprocess

import numpy as np

import rvcp_amd
from test_jit_cpu import PRELUDE, TRI_DTYPE, _scan_source, _tri_records

f32 = np.float32

GROUP_PRELUDE = r"""
#include <cmath>
static int g_rcp_mode = 0;
static inline float box_rcp(float x) {
    float r = 1.0f / x;
    if (g_rcp_mode != 0 && std::isfinite(r) && r != 0.0f)
        r = std::nextafterf(r, g_rcp_mode > 0 ? INFINITY : -INFINITY);
    return r;
}
#define RVCP_SPEC_BOX_RCP(x) box_rcp(x)
"""

# the kernel's per-wave guard (rvcp_kernels.hip ray_in_range with dir_grain_ok), the reference
# test in the numeric contract's operation order (cross_i = fma(a_j, b_k, -(a_k
# b_j)), dot = fma(z, z', fma(y, y', x x'))), and the three scans of every ray
GROUP_DRIVER = r"""
static inline bool ray_in_range(f3 o, f3 d) {
    return ((std::fabs(o.x) + std::fabs(o.y)) + std::fabs(o.z)) <= 0x1p41f &&
           ((std::fabs(d.x) + std::fabs(d.y)) + std::fabs(d.z)) <= 16.0f && dir_grain_ok(d);
}
static inline f3 crossf(f3 a, f3 b) {
    return f3{std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)),
              std::fmaf(a.x, b.y, -(a.y * b.x))};
}
static inline float dotf(f3 a, f3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
static void reference(const float *tri, int n_tri, f3 o, f3 d, float tmin, float &bt, int &best) {
    for (int i = 0; i < n_tri; i++) {
        const float *T = tri + 12 * i;
        const f3 v0{T[0], T[1], T[2]}, e1{T[3], T[4], T[5]}, e2{T[6], T[7], T[8]};
        const f3 s{o.x - v0.x, o.y - v0.y, o.z - v0.z};
        const f3 s1 = crossf(d, e2), s2 = crossf(s, e1);
        const float f = 1.0f / dotf(s1, e1);
        const float t = f * dotf(s2, e2), b1 = f * dotf(s1, s), b2 = f * dotf(s2, d);
        if ((b1 >= 0.0f) & (b2 >= 0.0f) & (b1 + b2 <= 1.0f) & (t >= tmin) & (t <= bt)) { bt = t; best = i; }
    }
}
// out[r]: t and face of the grouped scan's path slot, t of its shadow slot, the same of the
// ungrouped scan and of the reference loop; flags[r]: bit 1 the ray is within ray_in_range (the
// ungrouped scan ran), bit 0 it also passed the grouped scan's guard (else the kernel's wave
// takes the generic scan and nothing grouped runs); counts: rays that passed,
// (ray, group) pairs, pairs culled
extern "C" void groups_all(const float *tri, int n_tri, const float *rays, int n, float tmin,
                           float tmax, int rcp_mode, float *t_out, int *face_out, int *flags,
                           long *counts) {
    g_rcp_mode = rcp_mode;
    for (int r = 0; r < n; r++) {
        const float *q = rays + 6 * r;
        const f3 o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
        g_grain_ok = dir_grain_ok(d);
        float *t = t_out + 5 * r;
        int *fc = face_out + 3 * r;
        t[3] = tmax; fc[1] = -1;
        t[4] = tmax; fc[2] = -1;
        reference(tri, n_tri, o, d, tmin, t[4], fc[2]);
        flags[r] = 0;
        t[0] = t[1] = t[2] = tmax; fc[0] = -1;
        if (!ray_in_range(o, d)) continue;          // (the ungrouped scan's own premise)
        flags[r] = 2;
        spec_scan1(o, d, tmin, t[3], fc[1]);
#ifdef RVCP_SPEC_GROUPS
        if (!spec_group_origin_ok(o)) continue;
        flags[r] |= 1;
        counts[0] += 1;
        {   // the path slot (compact scan, and slot B of the dual scan below)
            float bt = tmax; int best = -1;
            spec_always1(o, d, tmin, bt, best);
            const unsigned m = spec_group_reach(o, d, tmin, bt);
            const float bound = bt;
            for (int g = 0; g < RVCP_SPEC_GROUPS; g++) {
                counts[1] += 1;
                if (!((m >> g) & 1u)) { counts[2] += 1; continue; }
                float ot = bound; int ob = -1;
                spec_group_scan(g, o, d, tmin, ot, ob);
                if (ob >= 0 && (ot < bt || (ot == bt && ob > best))) { bt = ot; best = ob; }
            }
            t[0] = bt; fc[0] = best;
        }
        {   // the dual scan: this ray in the shadow slot A, another ray in slot B -- and this
            // ray in slot B, whose result must be the path slot's above
            const f3 o2{q[0] + 1.0f, q[1], q[2]}, d2{q[4], q[5], q[3]};
            float btA = tmax, btB = tmax; int bestB = -1;
            spec_always2(o, d, o2, d2, tmin, btA, btB, bestB);
            const unsigned m = spec_group_reach(o, d, tmin, btA);
            const float bound = btA;
            for (int g = 0; g < RVCP_SPEC_GROUPS; g++) {
                if (!((m >> g) & 1u)) continue;
                float ot = bound; int ob = -1;
                spec_group_scan(g, o, d, tmin, ot, ob);
                if (ob >= 0 && ot < btA) btA = ot;
            }
            t[1] = btA;
            float btA2 = tmax, btB2 = tmax; int bestB2 = -1;
            spec_always2(o2, d2, o, d, tmin, btA2, btB2, bestB2);
            const unsigned m2 = spec_group_reach(o, d, tmin, btB2);
            const float bound2 = btB2;
            for (int g = 0; g < RVCP_SPEC_GROUPS; g++) {
                if (!((m2 >> g) & 1u)) continue;
                float ot = bound2; int ob = -1;
                spec_group_scan(g, o, d, tmin, ot, ob);
                if (ob >= 0 && (ot < btB2 || (ot == btB2 && ob > bestB2))) { btB2 = ot; bestB2 = ob; }
            }
            t[2] = btB2;
            if (bestB2 != fc[0]) fc[0] = -2;        // the two forms disagree: a mismatch
        }
#endif
    }
}
extern "C" int n_groups() {
#ifdef RVCP_SPEC_GROUPS
    return RVCP_SPEC_GROUPS;
#else
    return 0;
#endif
}
"""


def positions(sc):
    V = sc.mesh.aligned_vertices()["position"][:, :3]
    return np.ascontiguousarray(V[sc.mesh.aligned_faces()["vertices"]], dtype=f32)


def lum_mask(sc):
    m = 0
    for i in sc.luminous_face_ids():
        m |= 1 << int(i)
    return m


def groups_source(rec, mask):
    L = rvcp_amd.abi.load()
    fn = L.rvcp_internal_jit_groups_source
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    n = fn(rec.ctypes.data, len(rec), mask, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    fn(rec.ctypes.data, len(rec), mask, buf, n + 1)
    return buf.value.decode()


def partition(rec, mask):
    """(group_of [F] int32, boxes [G, 2, 3] float32) of rvcp_jit.cpp's jit_scan_groups."""
    L = rvcp_amd.abi.load()
    fn = L.rvcp_internal_jit_groups
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    group_of = np.zeros(len(rec), np.int32)
    box = np.zeros((4, 2, 3), f32)
    n = fn(rec.ctypes.data, len(rec), mask, group_of.ctypes.data, box.ctypes.data)
    assert n >= 0
    return group_of, box[:n]


class GroupedScan:
    """The generated scans of a scene, compiled for the CPU."""

    def __init__(self, tmp_path, sc, name):
        self.pos = positions(sc)
        self.rec = _tri_records(self.pos)
        assert self.rec.dtype == TRI_DTYPE
        self.mask = lum_mask(sc)
        self.text = groups_source(self.rec, self.mask)
        src = tmp_path / f"{name}.cpp"
        src.write_text(PRELUDE + GROUP_PRELUDE + _scan_source(self.rec) + self.text + GROUP_DRIVER)
        so = tmp_path / f"{name}.so"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-mfma", "-fno-fast-math", "-o", str(so), str(src)], check=True)
        self.lib = ctypes.CDLL(str(so))
        self.lib.groups_all.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self.n_groups = int(self.lib.n_groups())

    def run(self, rays, tmin, tmax, rcp_mode=0):
        """(t [R, 5] float32, face [R, 3] int32, flags [R] int32, counts [3]): see groups_all."""
        rays = np.ascontiguousarray(rays, dtype=f32)
        n = len(rays)
        t = np.zeros((n, 5), f32)
        face = np.zeros((n, 3), np.int32)
        flags = np.zeros(n, np.int32)
        counts = np.zeros(3, np.int64)
        self.lib.groups_all(self.rec.ctypes.data, len(self.rec), rays.ctypes.data, n, tmin, tmax,
                            rcp_mode, t.ctypes.data, face.ctypes.data, flags.ctypes.data,
                            counts.ctypes.data)
        return t, face, flags, counts


# ---------------------------------------------------------------------------------- scenes
def _with_box(sc, base_xz, height):
    """`sc` plus a box (top and four sides, ten faces of material 0) standing on y = 0 over the
    quadrilateral base_xz, built as the Cornell box's own boxes are."""
    V = sc.mesh.aligned_vertices().copy()
    F = sc.mesh.aligned_faces().copy()
    b = [np.array([x, 0.0, z], f32) for x, z in base_xz]
    lift = np.array([0.0, height, 0.0], f32)
    quads = [([p + lift for p in b], np.array([0, 1, 0], f32))]
    for i in range(4):
        p, q = b[i], b[(i + 1) % 4]
        n = np.cross((q - p).astype(np.float64), [0.0, 1.0, 0.0])
        quads.append(([p, q, q + lift, p + lift], (n / np.linalg.norm(n)).astype(f32)))
    nv = np.zeros(4 * len(quads), V.dtype)
    nf = np.zeros(2 * len(quads), F.dtype)
    for k, (ps, n) in enumerate(quads):
        for j, p in enumerate(ps):
            nv["position"][4 * k + j, :3] = p
            nv["normal"][4 * k + j, :3] = n
        base = len(V) + 4 * k
        nf["vertices"][2 * k] = (base, base + 1, base + 2)
        nf["vertices"][2 * k + 1] = (base, base + 2, base + 3)
    mesh = rvcp_amd.scene.ArrayMesh(np.concatenate([V, nv]), np.concatenate([F, nf]))
    return rvcp_amd.Scene(sc.camera, list(sc.materials), list(sc.spheres), mesh)


def three_box_scene(base=None):
    """The Cornell box plus a third box in the free corner of its floor: 42 faces, three groups."""
    c, r, a = np.array([160.0, -160.0]), 60.0, np.radians(30.0)
    base_xz = [c + r * np.array([np.cos(a + k * np.pi / 2), np.sin(a + k * np.pi / 2)]) for k in (3, 2, 1, 0)]
    return _with_box(base or rvcp_amd.Scene.default(), base_xz, 110.0)


def crowded_scene():
    """The overflow scene: the Cornell box with its tall box widened about its centre as far as
    the surface-area rule admits (1.08 x in x and z, still inside the room) plus the third box, so
    that a wave's rays reach more (ray, group) pairs than one pass of 64 holds."""
    sc = rvcp_amd.Scene.default()
    V = sc.mesh.aligned_vertices().copy()
    F = sc.mesh.aligned_faces()["vertices"]
    ids = np.unique(F[12:22])
    p = V["position"][ids, :3].astype(np.float64)
    c = 0.5 * (p.min(0) + p.max(0))
    p[:, 0] = c[0] + 1.08 * (p[:, 0] - c[0])
    p[:, 2] = c[2] + 1.08 * (p[:, 2] - c[2])
    V["position"][ids, :3] = p.astype(f32)
    mesh = rvcp_amd.scene.ArrayMesh(V, sc.mesh.aligned_faces().copy())
    return three_box_scene(rvcp_amd.Scene(sc.camera, list(sc.materials), list(sc.spheres), mesh))
