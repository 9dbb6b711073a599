"""librvcp's frame plan on the CPU, under AddressSanitizer / UBSan.

csrc/rvcp_frame_plan.cpp holds what a render decides before it touches the device: the
kernel schedule (the automatic choice among 3 / 5 / 6 / 10, the BVH, mode 2, the black frame),
which scene-specialised kernels replace built-in ones, and the persistent grid.  It is built
here with g++ -fsanitize=address,undefined from that file alone, together with
tools/frame_plan_check.cpp, and held against tests/frame_plan_ref.py -- the same decision
written independently in Python -- over the cross product below, in one process.  The named
assertions are derived from the code and the comments of csrc/rvcp_internal.h, not from either
transcription, so a mistake both share still fails."""
import itertools
import os
import shutil
import subprocess

import pytest

import frame_plan_ref as R
from rvcp_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc")
K = R.constants()
SPEC = abi.VARIANT_SPECIALIZED
SMALL = (47 * 39, 2)                    # (pixels, spp) of the small frame


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("plan") / "frame_plan_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tools", "frame_plan_check.cpp"),
                        os.path.join(CSRC, "rvcp_frame_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build unavailable: " + r.stderr[-300:])
    return exe


def _run(exe, lines, tmp_path):
    """The checker's output lines for the input lines (an iterable): one process, through files,
    with no sanitizer report."""
    src, dst = tmp_path / "plan_in.txt", tmp_path / "plan_out.txt"
    with open(src, "w") as f:
        n = sum(f.write(ln + "\n") > 0 for ln in lines)
    with open(src) as fin, open(dst, "w") as fout:
        r = subprocess.run([exe], stdin=fin, stdout=fout, stderr=subprocess.PIPE, text=True,
                           timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    out = dst.read_text().split("\n")
    assert out.pop() == "" and len(out) == n
    return out


def _frames():
    """(pixels, spp, stride) of the cross product: one below, at and one above each
    pixel-sample threshold (one sample per pixel), the small frame, and an empty shard."""
    out = []
    for name in ("kTiledDualMinSamples", "kWideMinSamples", "kSpecWideMinSamples"):
        out += [(K[name] + d, 1, K[name] + d) for d in (-1, 0, 1)]
    return out + [SMALL + SMALL[:1], (0, 2, 47 * 8)]


def _cross_product():
    games, legacy = abi.INTEGRATOR_GAMES101, abi.INTEGRATOR_LEGACY
    # the BVH with games101 only: rvcp_create refuses the other
    routes = ((games, abi.ACCEL_NONE), (games, abi.ACCEL_BVH), (legacy, abi.ACCEL_NONE))
    for (integrator, accel), module in itertools.product(routes, R.MODULES):
        base = R.make_input(module, integrator=integrator, accel=accel)
        for kv, faces, (px, spp, stride), t_min, bounces, att, n_frames, gwps, prefix in \
                itertools.product((0, 1, 2, 3, 4, 5, 6, 10), (0, 1, 32, 64, 65, 255, 256, 342),
                                  _frames(), (0.0, 1e-3), (0, 5), (0.01, 1.5), (1, 3), (0, 1, 4),
                                  (0, 12)):
            inp = dict(base)
            inp.update(kernel_variant=kv, n_faces=faces, frame_px=px, spp=spp, stride=stride,
                       ray_t_min=t_min, max_bounces=bounces, attenuation_stop_eps=att,
                       n_frames=n_frames, grid_waves_per_simd=gwps, bvh_prefix=prefix)
            yield inp


def _check_properties(inp, P):
    """What must hold of any plan, from the code and the header's comments."""
    legacy = inp["integrator"] == abi.INTEGRATOR_LEGACY
    bvh = inp["accel"] == abi.ACCEL_BVH and inp["n_faces"] > 0
    # an explicit schedule always wins, except under the BVH, which forces 3 (stats code 7)
    if bvh:
        assert P["variant"] == 3 and P["stats_code"] & ~SPEC in (0, 7)
    elif inp["kernel_variant"]:
        assert P["variant"] == inp["kernel_variant"]
    # a black frame: stats code 0, never a refused batch
    trivial = inp["max_bounces"] == 0 or (not legacy and inp["attenuation_stop_eps"] > 1.0)
    assert P["trivial"] == trivial
    if trivial:
        assert P["status"] == abi.RVCP_OK and P["stats_code"] == 0
    # a batch that is not black needs a pre-pass schedule of games101, or mode 2
    refused = inp["n_frames"] > 1 and not trivial and not legacy and P["variant"] in (1, 2)
    assert P["status"] == (abi.RVCP_E_UNSUPPORTED if refused else abi.RVCP_OK)
    if refused or trivial or inp["frame_px"] == 0:
        assert P["stats_code"] == 0 and P["blocks"] == 0
        return
    assert P["stats_code"] & ~SPEC == (8 if legacy else 7 if bvh else P["variant"])
    assert 1 <= P["blocks"] <= P["cap"]
    # schedule 10's workgroup is kTiledPoolWaves waves, every other kBlock threads
    pool = not legacy and not bvh and P["variant"] == K["kTiledPoolVariant"]
    assert P["wpb"] == (K["kTiledPoolWaves"] if pool else K["kBlock"] // K["kWave"])
    # a specialised kernel's grid is its own occupancy (CUs = SIMDs / 4), under the caller's limit
    n_spec = P["spec"] + P["spec_bvh"] + P["spec_legacy"]
    assert n_spec <= 1 and bool(P["stats_code"] & SPEC) == bool(n_spec)
    if n_spec:
        per_cu = (inp["blocks_per_cu_legacy"] if P["spec_legacy"] else inp["blocks_per_cu_bvh"]
                  if P["spec_bvh"] else inp["blocks_per_cu6"] if P["variant"] == 6
                  else inp["blocks_per_cu5"])
        assert per_cu > 0 and inp["module"]
        cap = per_cu * inp["n_simds"] // 4
        if inp["grid_waves_per_simd"]:
            cap = min(cap, max(1, inp["grid_waves_per_simd"] * inp["n_simds"] // P["wpb"]))
        assert P["cap"] == cap
    waves, chunk = R.static_split(inp["n_frames"] * inp["frame_px"], P["cap"] * P["wpb"],
                                  inp["n_simds"])
    assert (P["static_chunk"], P["static_chunks"]) == (chunk, waves * chunk)


def test_agrees_with_reference_on_cross_product(checker, tmp_path):
    want = []

    def lines():
        for inp in _cross_product():
            ref = R.plan(inp)
            want.append(" ".join(str(ref[f]) for f in R.OUT_FIELDS))
            yield R.line(inp)

    got = _run(checker, lines(), tmp_path)
    assert len(got) == 3 * 4 * 8 * 8 * 11 * 2 * 2 * 2 * 2 * 3 * 2
    for inp, ref, out in zip(_cross_product(), want, got):
        assert out == ref, (inp, dict(zip(R.OUT_FIELDS, zip(out.split(), ref.split()))))
        _check_properties(inp, dict(zip(R.OUT_FIELDS, map(int, out.split()))))


def test_thresholds_flip_automatic_schedule_at_their_value(checker, tmp_path):
    dual, wide, spec_wide = K["kTiledDualMinSamples"], K["kWideMinSamples"], K["kSpecWideMinSamples"]
    f_tiled, f_wide = K["kTiledMinFaces"], K["kTiledWideMinFaces"]
    assert dual < wide < spec_wide and f_wide < f_tiled
    generic = dict(ray_t_min=0.0)           # a module, but no specialised scan: t_min must be > 0
    # (module, faces, pixel-samples, further input) -> the automatic schedule
    cases = [
        # kTiledMinFaces: the tiled schedules from that many faces, whatever the frame's size
        ("absent", f_tiled - 1, dual - 1, {}, 3), ("absent", f_tiled, dual - 1, {}, 5),
        ("complete", f_tiled - 1, dual, {}, 3), ("complete", f_tiled, dual, {}, 10),
        # kTiledDualMinSamples: 5 below it, 10 from it on
        ("absent", 342, dual - 1, {}, 5), ("absent", 342, dual, {}, 10),
        # kTiledWideMinFaces: 10 ABOVE that many faces on such frames, with the generic scan only
        ("absent", f_wide, dual, {}, 3), ("absent", f_wide + 1, dual, {}, 10),
        ("absent", f_wide + 1, dual - 1, {}, 3), ("complete", f_wide + 1, dual, {}, 3),
        ("complete", f_wide + 1, dual, generic, 10),
        # kWideMinSamples: 6 from it on with the generic scan ...
        ("absent", 32, wide - 1, {}, 3), ("absent", 32, wide, {}, 6),
        ("complete", 32, wide - 1, generic, 3), ("complete", 32, wide, generic, 6),
        # ... kSpecWideMinSamples: and only from there with the specialised one
        ("complete", 32, wide, {}, 3), ("complete", 32, spec_wide - 1, {}, 3),
        ("complete", 32, spec_wide, {}, 6), ("absent", 32, spec_wide, {}, 6),
    ]
    inputs = [R.make_input(m, n_faces=f, frame_px=s, stride=s, **kw) for m, f, s, kw, _ in cases]
    got = _run(checker, [R.line(i) for i in inputs], tmp_path)
    for case, out in zip(cases, got):
        assert int(out.split()[R.OUT_FIELDS.index("variant")]) == case[-1], (case, out)


def test_static_split_agrees(checker, tmp_path):
    """static_split of csrc/rvcp_internal.h, as a plain g++ program sees it, against the rule of
    its comment."""
    cases = [(n, g, s) for n in (0, 1, 7, 8, 9, 63, 64, 65, 1833, 5499, 16383, 16384, 1 << 19,
                                 (1 << 28) + 1, 3 * ((1 << 28) + 1))
             for g in (1, 4, 256, 5120, 20480) for s in (4, 1024)]
    got = _run(checker, ["split %d %d %d" % c for c in cases], tmp_path)
    for c, out in zip(cases, got):
        assert tuple(map(int, out.split())) == R.static_split(*c), c
        waves, chunk = map(int, out.split())
        assert 1 <= waves <= max(1, c[1]) and 1 <= chunk <= K["kChunk"]
        if waves < c[1] and c[0]:
            assert waves * chunk >= c[0]        # the static chunks cover a queue the grid can hold
