"""The item layout of the grouped scan's passes (csrc/rvcp_group_pack.h; DESIGN.md §4.7 "Face
groups"), checked on the CPU.

The header is plain C++: it is compiled with g++ into a small shared object behind an array
driver, and for every vector of per-group item counts c[g] (G <= 4, each <= 128):

    every item gets a distinct (pass, lane), lane < 64, pass < the stated number of passes;
    the occupied lanes of every pass are a prefix of the stated length, and no pass is empty;
    scans (one per group a pass holds) = sum ceil(c / 64), the minimum;
    one pass when there are 64 items or fewer in all;
    cost = 270 scans + 100 passes (the weights of DESIGN.md §4.7) is at most the cost of the
    contiguous numbering -- groups one after the other without padding, cut every 64 --
    re-implemented here in numpy from that description.

Inputs: G = 2, every (c0, c1) in 0..128 x 0..128; G = 3, every triple in 0..70, plus 100 000
seeded random vectors up to 128; G = 4, 100 000 seeded random vectors up to 128; and for G = 2
every A/B split of each count up to 20 items, item by item through rvcp_group_pack_item.

Second part: the conditions the GPU cases of tests/test_gpu_group_pack.py rest on -- the close
camera (tests/group_pack_cases.py) sees only the tall box, and every ray that starts on the tall
box's faces reaches that box's group."""
import ctypes
import subprocess

import numpy as np
import pytest

import rvcp_amd
from group_pack_cases import TALL_BOX_FACES, close_camera_scene, reach_masks
from spec_groups import GroupedScan, crowded_scene, partition

SCAN_COST, PASS_COST = 270, 100
MAX_PASSES = 8          # sum ceil(c / 64) <= 2 G

DRIVER = r"""
#include "rvcp_group_pack.h"
extern "C" void pack_all(const uint32_t *c, int n, int G, uint32_t *start, uint32_t *passes,
                         uint32_t *lanes) {
    for (int i = 0; i < n; i++) {
        passes[i] = rvcp_group_pack(c + 4 * i, G, start + 4 * i);
        for (uint32_t p = 0; p < 8; p++)
            lanes[8 * i + p] = p < passes[i] ? rvcp_group_pack_lanes(c + 4 * i, start + 4 * i, G, p) : 0u;
    }
}
// in_pass / span of one group in one pass, and an item's index
extern "C" int in_pass(uint32_t c, uint32_t start, uint32_t p) { return rvcp_group_pack_in_pass(c, start, p); }
extern "C" void span(uint32_t c, uint32_t start, uint32_t p, uint32_t *lo, uint32_t *hi) {
    rvcp_group_pack_span(c, start, p, lo, hi);
}
extern "C" uint32_t item(uint32_t start, uint32_t n_a, int slot_b, uint32_t rank) {
    return rvcp_group_pack_item(start, n_a, slot_b, rank);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    import os
    d = tmp_path_factory.mktemp("group_pack")
    csrc = os.path.join(os.path.dirname(os.path.abspath(rvcp_amd.abi.__file__)), "csrc")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    so = d / "group_pack.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", csrc,
                    "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    L.pack_all.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.in_pass.argtypes = [ctypes.c_uint32] * 3
    L.span.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 2
    L.item.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
    L.item.restype = ctypes.c_uint32
    return L


def _pack(lib, counts):
    """(start [N, 4], passes [N], lanes [N, 8]) of the header for counts [N, G]."""
    n, G = counts.shape
    c = np.zeros((n, 4), np.uint32)
    c[:, :G] = counts
    start = np.zeros((n, 4), np.uint32)
    passes = np.zeros(n, np.uint32)
    lanes = np.zeros((n, 8), np.uint32)
    lib.pack_all(c.ctypes.data, n, G, start.ctypes.data, passes.ctypes.data, lanes.ctypes.data)
    return start[:, :G].astype(np.int64), passes.astype(np.int64), lanes.astype(np.int64)


def _overlap(s, e, p):
    """Items of [s, e) in pass p ([64 p, 64 p + 64)), elementwise."""
    return np.clip(np.minimum(e, 64 * p + 64) - np.maximum(s, 64 * p), 0, None)


def _contiguous(counts):
    """The parent's numbering: (scans, passes)."""
    c = counts.astype(np.int64)
    e = np.cumsum(c, axis=1)
    s = e - c
    passes = (e[:, -1] + 63) // 64
    scans = np.zeros(len(c), np.int64)
    for p in range(MAX_PASSES):
        scans += (_overlap(s, e, p) > 0).sum(axis=1)
    return scans, passes


def _check(lib, counts):
    c = counts.astype(np.int64)
    n, G = c.shape
    start, passes, lanes = _pack(lib, counts)
    end = start + c
    total = c.sum(axis=1)
    some = c > 0
    # distinct (pass, lane): the non-empty groups' index ranges are disjoint and inside the passes
    for g in range(G):
        for h in range(g + 1, G):
            both = some[:, g] & some[:, h]
            assert np.all(~both | (end[:, g] <= start[:, h]) | (end[:, h] <= start[:, g]))
    assert np.all(~some | (end <= 64 * passes[:, None]))
    assert np.all(passes <= MAX_PASSES)
    # the occupied lanes of each pass: a prefix of the stated length, never empty
    scans = np.zeros(n, np.int64)
    for p in range(MAX_PASSES):
        ov = np.where(some, _overlap(start, end, p), 0)
        held = ov > 0
        filled = ov.sum(axis=1)
        top = np.where(held, np.minimum(end, 64 * p + 64) - 64 * p, 0).max(axis=1)
        live = p < passes
        assert np.all(lanes[:, p] == np.where(live, filled, 0))
        assert np.all(filled == top)                    # no hole below the topmost item
        assert np.all(~live | (filled > 0))
        assert np.all(live | (filled == 0))
        scans += held.sum(axis=1)
    assert np.array_equal(scans, ((c + 63) // 64).sum(axis=1))
    assert np.all(passes[total <= 64] == (total[total <= 64] > 0))
    ref_scans, ref_passes = _contiguous(counts)
    cost = SCAN_COST * scans + PASS_COST * passes
    ref = SCAN_COST * ref_scans + PASS_COST * ref_passes
    worse = cost > ref
    assert not worse.any(), (counts[worse][:5], cost[worse][:5], ref[worse][:5])
    return scans, passes, ref_scans, ref_passes


def test_two_groups_every_pair(lib):
    a = np.arange(129)
    counts = np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1).reshape(-1, 2)
    scans, passes, ref_scans, ref_passes = _check(lib, counts)
    # the issue's example: 45 + 30 items, two scans instead of three in the same two passes
    i = 45 * 129 + 30
    assert (scans[i], passes[i], ref_scans[i], ref_passes[i]) == (2, 2, 3, 2)


def test_three_groups_every_triple_to_70(lib):
    a = np.arange(71)
    _check(lib, np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


@pytest.mark.parametrize("G", [3, 4])
def test_random_vectors(lib, G):
    rng = np.random.default_rng(20260 + G)
    _check(lib, rng.integers(0, 129, (100_000, G)))


def _check_items(lib, c0, c1, splits0, splits1):
    lo, hi = ctypes.c_uint32(), ctypes.c_uint32()
    start, passes, lanes = _pack(lib, np.array([[c0, c1]]))
    for a0 in splits0:
        for a1 in splits1:
            seen = set()
            for g, (c, na) in enumerate(((c0, a0), (c1, a1))):
                s = int(start[0, g])
                idx = [lib.item(s, na, 0, r) for r in range(na)] + \
                      [lib.item(s, na, 1, r) for r in range(c - na)]
                assert idx == list(range(s, s + c))
                for v in idx:
                    p, lane = v >> 6, v & 63
                    assert p < passes[0] and lane < lanes[0, p]
                    assert lib.in_pass(c, s, p)
                    lib.span(c, s, p, ctypes.byref(lo), ctypes.byref(hi))
                    assert lo.value <= lane < hi.value <= 64
                seen.update(idx)
            assert len(seen) == c0 + c1


def test_every_split_item_by_item(lib):
    """G = 2, counts up to 20 each, every (nA, nB) split of both: each item through
    rvcp_group_pack_item lands in its group's range, A first, all indices distinct, and in the
    lanes rvcp_group_pack_span states for its pass.  Then the same with the extreme and middle
    splits of counts that pad (45 + 30), fill a pass exactly, and span two passes each."""
    for c0 in range(21):
        for c1 in range(21):
            _check_items(lib, c0, c1, range(c0 + 1), range(c1 + 1))
    for c0, c1 in ((45, 30), (64, 1), (1, 64), (63, 2), (100, 60), (65, 64), (128, 128)):
        _check_items(lib, c0, c1, (0, c0 // 2, c0), (0, c1 // 2, c1))


# ------------------------------------------------- the premise of the GPU cases
@pytest.mark.parametrize("name", ["cornell", "crowded"])
def test_rays_from_the_tall_box_all_reach_its_group(tmp_path, name):
    """From points on the tall box's faces, rays in every direction reach the tall box's group
    (group 0) whatever their bound, with the slab reciprocal at the IEEE quotient and 1 ulp either
    side: a full wave of the close-camera frame -- 64 shadow and up to 64 path rays from such
    points -- holds more than 64 items of that one group."""
    base = rvcp_amd.Scene.default() if name == "cornell" else crowded_scene()
    gs = GroupedScan(tmp_path, close_camera_scene(base), name)
    group_of, _ = partition(gs.rec, gs.mask)
    assert [int(group_of[f]) for f in TALL_BOX_FACES] == [0] * len(TALL_BOX_FACES)
    rng = np.random.default_rng(7)
    p = gs.pos[list(TALL_BOX_FACES)].astype(np.float64)
    n = 50_000
    f = rng.integers(0, len(p), n)
    o = np.einsum("rk,rkc->rc", rng.dirichlet([1.0, 1.0, 1.0], n), p[f])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1)
    for bound in (10000.0, 1.0):            # t_max, and a bound just above t_min = 0.01
        for mode in (0, 1, -1):
            mask = reach_masks(tmp_path, gs, name, rays, 0.01, bound, mode)
            assert np.all(mask >= 0) and np.all(mask & 1), (bound, mode, int((mask & 1 == 0).sum()))


def test_the_close_camera_sees_only_the_tall_box():
    """Every primary ray of the 416 x 320 close-camera frame lands on a face of the tall box:
    the frame's corner directions hit the camera-facing side inside its outline."""
    sc = close_camera_scene(rvcp_amd.Scene.default())
    cam = sc.camera
    pos = cam.position.astype(np.float64)
    fwd, up, right = (np.asarray(v, np.float64) for v in (cam.forward, cam.up, cam.right))
    th = np.tan(np.radians(cam.vertical_fov) / 2.0)
    a, b = np.array([148.0, 0.0, -28.0]), np.array([-10.0, 0.0, 21.0])     # the side's base edge
    nrm = np.cross(b - a, [0.0, 1.0, 0.0])
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            d = fwd + sx * th * (416.0 / 320.0) * right + sy * th * up
            t = np.dot(a - pos, nrm) / np.dot(d, nrm)
            q = pos + t * d
            u = np.dot(q - a, b - a) / np.dot(b - a, b - a)
            assert t > 0 and 0.05 < u < 0.95 and 10.0 < q[1] < 320.0, (sx, sy, q)
