// Build: g++ -O2 -std=c++17 -ffp-contract=off -I rvcp-real-time-path-tracer_amd/csrc tools/bvh4_check.cpp \
//          rvcp-real-time-path-tracer_amd/csrc/rvcp_bvh.cpp -o /tmp/bvh4_check
// Input: raw float32 triangles [n][3][3] (e.g. the C5 mesh written by tools/dump_mesh.py).
// CPU check of the real builder + collapse: stack bound, node count, traversal steps, and that
// BVH4 traversal finds the same nearest hit as brute force on random rays.  A third argument
// `hybrid` checks the BVH hybrid instead (rvcp_host.cpp upload_one): the leading large faces
// (bvh_big_prefix) tested by brute force first, the BVH built over the rest.
//
// Rays mode: bvh4_check MESH rays RAYS OUT [hybrid] [noslack]
// RAYS holds float32 records {o[3], d[3], t_min, t_max}; every ray is traced three ways -- brute
// force, the float-node traversal (trav_float, IEEE reciprocals) and the traversal over the
// byte-quantised nodes in the device's own arithmetic form and operation order (trav_quant,
// copied from bvh_nearest in rvcp_kernels.hip) -- and OUT receives per ray the little-endian
// record {int32 face, float t} x {brute, float nodes, quantised nodes} (face -1: a miss, t then
// the ray's t_max).  The line `pad_abs` prints the builder's own absolute box pad as a hex
// float; tests/bvh_adversarial.py classifies the disagreements.  Exit status 0 whenever the
// traversals ran within the stack bound (the deepest stack either traversal reached against
// bvh4_collapse's bound): disagreements are the caller's to judge.  In rays mode both
// traversals compare slabs with the relative slack of the device's primary rays (kBvhSlabSlack);
// and key unused child slots (inverted bytes) +inf; `noslack` takes both out, which is the
// form of the shadow and path rays (bvh4_step) and of the random-ray mode above.
//
// -DBVH_CHECK_MUTATE=k plants one fault in this model (never in the product), to show that the
// tests that read it notice (tests/test_bvh_adversarial_cpu.py): 1 = boxes entered exactly at
// the nearest hit are culled (tn >= bt), 2 = the order rule without its tie half (t < bt),
// 3 = the quantised lower bounds rounded inward, 4 = the build's box enlargement taken back,
// 5 = unused child slots left to their inverted boxes alone (not keyed +inf) in the primary form.
// -DBVH_CHECK_FUSED=1 is no fault: the triangle test with the device's fused dot and cross (tri()).
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <random>
#include <algorithm>
#include <string>
#include "rvcp_internal.h"
using namespace rvcp;
#ifndef BVH_CHECK_MUTATE
#define BVH_CHECK_MUTATE 0
#endif
#ifndef BVH_CHECK_FUSED
#define BVH_CHECK_FUSED 0
#endif
std::vector<float> P;
static float g_slack = 0.0f;     // kBvhSlabSlack in rays mode unless `noslack` (the secondary rays' form)
static bool g_mask = false;      // unused slots keyed +inf: with the slack, the primary rays' form
static bool slab(const Bvh4Node &N, int i, const float *o, const float *inv, float tmin, float bt, float &tn_) {
    float tn = tmin, tf = bt;
    for (int k = 0; k < 3; k++) { float a = (N.lo[k][i] - o[k]) * inv[k], c = (N.hi[k][i] - o[k]) * inv[k]; tn = std::max(tn, std::min(a, c)); tf = std::min(tf, std::max(a, c)); }
    tn_ = tn;
    const float tfs = std::fmaf(std::fabs(tf), g_slack, tf);      // as the device (trav_quant)
#if BVH_CHECK_MUTATE == 1
    return tn <= tfs && tn < bt;
#else
    return tn <= tfs;
#endif
}
static float dot3(const float *a, const float *b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
static void cross3(const float *a, const float *b, float *c) {
    c[0] = std::fmaf(a[1], b[2], -(a[2] * b[1]));
    c[1] = std::fmaf(a[2], b[0], -(a[0] * b[2]));
    c[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
static bool tri(const float *v, const float *o, const float *d, float tmin, float bt, float &t) {
    float e1[3] = {v[3]-v[0], v[4]-v[1], v[5]-v[2]}, e2[3] = {v[6]-v[0], v[7]-v[1], v[8]-v[2]};
    float s[3] = {o[0]-v[0], o[1]-v[1], o[2]-v[2]};
#if BVH_CHECK_FUSED
    // -DBVH_CHECK_FUSED=1: dot and cross as the device's and the oracle's fused chains (DESIGN.md
    // §3.1), so that the brute column is the scan's own hit, bit for bit (tests/test_rays_cpu.py).
    // The default build keeps the unfused products every figure of DESIGN.md §4.6 was measured with.
    float s1[3], s2[3];
    cross3(d, e2, s1);
    cross3(s, e1, s2);
    float ff = 1 / dot3(s1, e1);
    t = ff * dot3(s2, e2);
    float b1 = ff * dot3(s1, s);
    float b2 = ff * dot3(s2, d);
#else
    float s1[3] = {d[1]*e2[2]-d[2]*e2[1], d[2]*e2[0]-d[0]*e2[2], d[0]*e2[1]-d[1]*e2[0]};
    float s2[3] = {s[1]*e1[2]-s[2]*e1[1], s[2]*e1[0]-s[0]*e1[2], s[0]*e1[1]-s[1]*e1[0]};
    float ff = 1 / (s1[0]*e1[0]+s1[1]*e1[1]+s1[2]*e1[2]);
    t = ff * (s2[0]*e2[0]+s2[1]*e2[1]+s2[2]*e2[2]);
    float b1 = ff * (s1[0]*s[0]+s1[1]*s[1]+s1[2]*s[2]);
    float b2 = ff * (s2[0]*d[0]+s2[1]*d[1]+s2[2]*d[2]);
#endif
    return b1 >= 0 && b2 >= 0 && b1 + b2 <= 1 && t >= tmin && t <= bt;
}
// the order rule of the leaf test (bvh_leaf): smaller t, or equal t and the later face
static bool keeps(float t, float bt, int id, int best) {
#if BVH_CHECK_MUTATE == 2
    (void)id; (void)best;
    return t < bt;
#else
    return t < bt || id > best;
#endif
}

struct Tree {
    std::vector<Bvh4Node> n4;
    std::vector<Bvh4QNode> q4;
    std::vector<uint32_t> order;
    int32_t r4 = 0;
};
struct Hit { int face; float t; };
static double g_steps = 0, g_tris = 0;
static int g_maxsp = 0;
static bool g_overflow = false;

static void leaf(const Tree &T, int32_t ref, const float *o, const float *d, float tmin, float &bt, int &best) {
    const uint32_t code = ~(uint32_t)ref, first = code >> 5, cnt = (code & 31) + 1;
    for (uint32_t q = 0; q < cnt; q++) {
        g_tris++; float t; const int id = (int)T.order[first + q];
        if (tri(&P[9 * (size_t)id], o, d, tmin, bt, t) && keeps(t, bt, id, best)) { bt = t; best = id; }
    }
}
// the 5-comparator child sort, the pushes (farthest first) and the descent of one node step
// (unused[i]: the slot holds no child; an entered one carries ~0, the leaf {slot 0, 1 triangle})
static bool step_children(float *k, int32_t *c, const bool *unused, int32_t *st, int &sp, int32_t &ref) {
#if BVH_CHECK_MUTATE != 5
    if (g_mask) for (int i = 0; i < 4; i++) if (unused[i]) k[i] = INFINITY;    // primary form: never entered
#else
    (void)unused;
#endif
    auto cas = [&](int a, int b) { if (k[b] < k[a]) { std::swap(k[a], k[b]); std::swap(c[a], c[b]); } };
    cas(0,1); cas(2,3); cas(0,2); cas(1,3); cas(1,2);
    for (int i = 3; i >= 1; i--) if (k[i] < INFINITY) { if (sp >= 64) { g_overflow = true; return false; } st[sp++] = c[i]; }
    g_maxsp = std::max(g_maxsp, sp);
    if (k[0] < INFINITY) { ref = c[0]; return true; }
    return false;
}
// Float-node traversal: the Bvh4Node boxes, IEEE reciprocals of the direction (a zero component
// gives +-inf, and inf * 0 = NaN drops out of std::max / std::min as written in slab()).
static Hit trav_float(const Tree &T, const float *o, const float *d, float tmin, float bt, int best) {
    const float inv[3] = {1 / d[0], 1 / d[1], 1 / d[2]};
    if (T.order.empty()) return {best, bt};
    int32_t st[64]; int sp = 0; int32_t ref = T.r4;
    for (;;) {
        g_steps++;
        if (ref >= 0) {
            const Bvh4Node &N = T.n4[ref]; float k[4]; int32_t c[4];
            bool un[4];
            for (int i = 0; i < 4; i++) { float tn; k[i] = slab(N, i, o, inv, tmin, bt, tn) ? tn : INFINITY; c[i] = N.ref[i]; un[i] = !N.pad[i]; }
            if (step_children(k, c, un, st, sp, ref)) continue;
        } else {
            leaf(T, ref, o, d, tmin, bt, best);
        }
        if (!sp) break; ref = st[--sp];
    }
    return {best, bt};
}
// The device's traversal (bvh_nearest, rvcp_kernels.hip) restated operation for operation over
// the Bvh4QNode array: slab_inv's substitution of 1e-30 for a zero direction component, the
// near and far bytes chosen by the sign of the inverse direction, every child bound decoded
// straight into slab time as fma(q, scale * inv, (origin - o) * inv), the fmax / fmin trees in
// the kernel's association (a NaN operand drops out, as in v_max_f32 / v_min_f32), entry iff
// tn <= tf + slack |tf| (primary rays; none for the others) with tf already clamped to bt (so
// only tn > bt culls), misses keyed +inf, unused slots (x bytes inverted) too in the primary
// form, and the leaf's order rule.  Two
// differences remain, and the GPU tests (tests/test_gpu_bvh_adversarial.py) are the authority
// for both: (1) the device takes the reciprocals with v_rcp_f32 (1 ulp),
// this model the IEEE quotient; (2) the device parks leaves and tests them a few node steps
// later (speculative while-while), so its culling sees a bt that is never below this model's.
static Hit trav_quant(const Tree &T, const float *o, const float *d, float tmin, float bt, int best) {
    const float inv[3] = {1.0f / (d[0] != 0.0f ? d[0] : 1e-30f), 1.0f / (d[1] != 0.0f ? d[1] : 1e-30f),
                          1.0f / (d[2] != 0.0f ? d[2] : 1e-30f)};
    const bool pos[3] = {inv[0] >= 0.0f, inv[1] >= 0.0f, inv[2] >= 0.0f};
    if (T.order.empty()) return {best, bt};
    int32_t st[64]; int sp = 0; int32_t ref = T.r4;
    for (;;) {
        g_steps++;
        if (ref >= 0) {
            const Bvh4QNode &N = T.q4[ref];
            float a[3], b[3]; uint32_t nb[3], fb[3];
            for (int k = 0; k < 3; k++) {
                a[k] = N.scale[k] * inv[k];
                b[k] = (N.origin[k] - o[k]) * inv[k];
                nb[k] = pos[k] ? N.qlo[k] : N.qhi[k];
                fb[k] = pos[k] ? N.qhi[k] : N.qlo[k];
            }
            float k[4]; int32_t c[4]; bool un[4];
            for (int i = 0; i < 4; i++) {
                auto by = [&](uint32_t w) { return (float)((w >> (8 * i)) & 0xFFu); };
                un[i] = !(by(N.qlo[0]) <= by(N.qhi[0]));       // the device's test: x bytes inverted
                const float tn = std::fmax(std::fmax(std::fmaf(by(nb[0]), a[0], b[0]), std::fmaf(by(nb[1]), a[1], b[1])),
                                           std::fmax(std::fmaf(by(nb[2]), a[2], b[2]), tmin));
                const float tf = std::fmin(std::fmin(std::fmaf(by(fb[0]), a[0], b[0]), std::fmaf(by(fb[1]), a[1], b[1])),
                                           std::fmin(std::fmaf(by(fb[2]), a[2], b[2]), bt));
                const float tfs = std::fmaf(std::fabs(tf), g_slack, tf);
#if BVH_CHECK_MUTATE == 1
                k[i] = tn <= tfs && tn < bt ? tn : INFINITY;
#else
                k[i] = tn <= tfs ? tn : INFINITY;
#endif
                c[i] = N.ref[i];
            }
            if (step_children(k, c, un, st, sp, ref)) continue;
        } else {
            leaf(T, ref, o, d, tmin, bt, best);
        }
        if (!sp) break; ref = st[--sp];
    }
    return {best, bt};
}
static Hit brute(uint32_t first, uint32_t n, const float *o, const float *d, float tmin, float bt, int best) {
    for (uint32_t i = first; i < n; i++) { float t; if (tri(&P[9 * (size_t)i], o, d, tmin, bt, t)) { bt = t; best = (int)i; } }
    return {best, bt};
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bvh4_check MESH [R [hybrid]] | MESH rays RAYS OUT [hybrid] [noslack]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); float buf[9];
    if (!f) { perror(argv[1]); return 2; }
    while (fread(buf, 4, 9, f) == 9) P.insert(P.end(), buf, buf + 9);
    fclose(f);
    uint32_t n = P.size() / 9; int32_t root;
    const bool rays_mode = argc > 4 && std::string(argv[2]) == "rays";
    const int hyb_arg = rays_mode ? 5 : 3;
    bool hybrid = false;
    if (rays_mode) { g_slack = kBvhSlabSlack; g_mask = true; }
    for (int i = hyb_arg; i < argc; i++) {
        if (std::string(argv[i]) == "hybrid") hybrid = true;
        if (std::string(argv[i]) == "noslack") { g_slack = 0.0f; g_mask = false; }
    }
    const uint32_t K = hybrid ? bvh_big_prefix((const float (*)[3][3])P.data(), n, kJitMaxFaces) : 0u;
    printf("prefix %u\n", K);
    std::vector<BvhNode> nodes; Tree T; float pad_abs = 0.0f;
    int depth = bvh_build((const float (*)[3][3])P.data() + K, n - K, nodes, T.order, root, &pad_abs);
    for (auto &id : T.order) if (id != kBvhPadId) id += K;
    std::vector<Bvh4Node> &n4 = T.n4;
    int need = bvh4_collapse(nodes, root, n4, T.r4);
    printf("n=%u nodes2=%zu depth=%d nodes4=%zu stack bound=%d\n", n, nodes.size(), depth, n4.size(), need);
    printf("pad_abs %a\n", (double)pad_abs);
#if BVH_CHECK_MUTATE == 4
    for (auto &N : n4)
        for (int c = 0; c < 4; c++) {
            if (!N.pad[c]) continue;
            for (int k = 0; k < 3; k++) {
                const float pad = pad_abs + 1e-6f * std::max(std::fabs(N.lo[k][c]), std::fabs(N.hi[k][c]));
                N.lo[k][c] += pad; N.hi[k][c] -= pad;
                if (N.lo[k][c] > N.hi[k][c]) N.lo[k][c] = N.hi[k][c] = 0.5f * (N.lo[k][c] + N.hi[k][c]);
            }
        }
#endif
    // bvh4_quantize: every used child's decoded box (exact, in double) contains its float box,
    // every unused child is inverted on all three axes, refs are copied
    std::vector<Bvh4QNode> &q4 = T.q4; bvh4_quantize(n4, q4); int qbad = 0; double grow = 0, ext = 0;
    for (size_t j = 0; j < n4.size(); j++)
        for (int c = 0; c < 4; c++) {
            qbad += q4[j].ref[c] != n4[j].ref[c];
            for (int k = 0; k < 3; k++) {
                const uint32_t ql = (q4[j].qlo[k] >> (8 * c)) & 255, qh = (q4[j].qhi[k] >> (8 * c)) & 255;
                const double lo = (double)q4[j].origin[k] + ql * (double)q4[j].scale[k];
                const double hi = (double)q4[j].origin[k] + qh * (double)q4[j].scale[k];
                if (!n4[j].pad[c]) { qbad += !(ql == 255 && qh == 0); continue; }
                qbad += !(lo <= n4[j].lo[k][c] && hi >= n4[j].hi[k][c]);
                grow += (hi - lo) - ((double)n4[j].hi[k][c] - n4[j].lo[k][c]);
                ext += (double)n4[j].hi[k][c] - n4[j].lo[k][c];
            }
        }
    printf("quantized: violations %d, box growth %.4f of extent\n", qbad, ext > 0 ? grow / ext : 0.0);
    if (qbad) return 1;
#if BVH_CHECK_MUTATE == 3
    for (auto &Q : q4)
        for (int c = 0; c < 4; c++) {
            if (!n4[&Q - q4.data()].pad[c]) continue;
            for (int k = 0; k < 3; k++) {
                const uint32_t ql = (Q.qlo[k] >> (8 * c)) & 255, qh = (Q.qhi[k] >> (8 * c)) & 255;
                if (ql < qh) Q.qlo[k] += 1u << (8 * c);
            }
        }
#endif
    if (rays_mode) {
        FILE *fr = fopen(argv[3], "rb"), *fo = fopen(argv[4], "wb");
        if (!fr || !fo) { perror("rays/out"); return 2; }
        float r[8]; int R = 0, badf = 0, badq = 0;
        while (fread(r, 4, 8, fr) == 8) {
            const float *o = r, *d = r + 3; const float tmin = r[6], tmax = r[7];
            const Hit p = brute(0, K, o, d, tmin, tmax, -1);        // the hybrid's prefix first
            const Hit hf = trav_float(T, o, d, tmin, p.t, p.face);
            const Hit hq = trav_quant(T, o, d, tmin, p.t, p.face);
            const Hit hb = brute(0, n, o, d, tmin, tmax, -1);
            const Hit out[3] = {hb, hf, hq};
            for (const Hit &h : out) { int32_t fc = h.face; fwrite(&fc, 4, 1, fo); fwrite(&h.t, 4, 1, fo); }
            badf += hf.face != hb.face || (hb.face >= 0 && hf.t != hb.t);
            badq += hq.face != hb.face || (hb.face >= 0 && hq.t != hb.t);
            R++;
        }
        fclose(fr);
        if (fclose(fo)) { perror("out"); return 2; }
        printf("rays %d float-node mismatches %d quantised mismatches %d max stack %d\n", R, badf, badq, g_maxsp);
        return g_overflow || need > kBvhStack || depth >= kBvhStack || g_maxsp > need;
    }
    std::mt19937 rng(1); std::uniform_real_distribution<float> U(0, 1);
    int R = argc > 2 ? atoi(argv[2]) : 5000, bad = 0;
    for (int r = 0; r < R; r++) {
        float o[3] = {-270 + 540 * U(rng), 0 + 548 * U(rng), -270 + 540 * U(rng)}; float d[3], l;
        do { for (int k = 0; k < 3; k++) d[k] = 2 * U(rng) - 1; l = d[0]*d[0]+d[1]*d[1]+d[2]*d[2]; } while (l > 1 || l < 1e-4);
        l = std::sqrt(l); for (int k = 0; k < 3; k++) d[k] /= l;
        const Hit p = brute(0, K, o, d, 1e-4f, 1e30f, -1);
        const Hit h = trav_float(T, o, d, 1e-4f, p.t, p.face);
        const Hit b = brute(0, n, o, d, 1e-4f, 1e30f, -1);
        if (b.face != h.face || (h.face >= 0 && b.t != h.t)) bad++;
    }
    printf("steps/ray %.1f tris/ray %.1f max stack %d mismatches %d of %d\n", g_steps / R, g_tris / R, g_maxsp, bad, R);
    return bad != 0 || need > kBvhStack || g_maxsp > need || g_overflow;
}
