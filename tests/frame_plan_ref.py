"""The frame plan in Python: what a render decides before it touches the device -- the kernel
schedule, the scene-specialised kernels that replace built-in ones, and the persistent grid.

Written from render_frames of csrc/rvcp_host.cpp as it stood before the decision moved into
csrc/rvcp_frame_plan.cpp, independently of that file; tests/test_frame_plan_cpu.py holds the two
against each other, tests/test_gpu_frame_plan.py holds real renders' stats against this one.
The thresholds are read from csrc/rvcp_internal.h as text.

Pure Python, no GPU (test infrastructure)."""
import functools
import os
import re

from rvcp_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL_H = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc", "rvcp_internal.h")

# one plan input, in the order tools/frame_plan_check.cpp reads a line
FIELDS = ("integrator", "kernel_variant", "accel", "spp", "max_bounces", "attenuation_stop_eps",
          "ray_t_min", "grid_waves_per_simd", "n_faces", "bvh_prefix", "n_simds",
          "grid_capacity",                  # eleven numbers, by schedule
          "bvh_capacity", "legacy_capacity", "module", "blocks_per_cu5", "blocks_per_cu6",
          "blocks_per_cu_bvh", "blocks_per_cu_legacy", "has_legacy", "has_bvh_path",
          "has_bvh_primary", "n_frames", "frame_px", "stride", "spread_min")
# ... and the plan, in the order it prints one
OUT_FIELDS = ("status", "variant", "accel", "trivial", "legacy", "spec", "spec_bvh", "spec_legacy",
              "cams", "prepass_batched", "out_px", "cap", "wpb", "blocks", "static_chunk",
              "static_chunks", "stats_code")

# a device of 256 CUs; resident workgroups per CU chosen all different, so that a plan that
# takes another kernel's capacity shows
N_SIMDS = 1024
GRID_CAPACITY = tuple(256 * n for n in (0, 7, 4, 5, 3, 8, 6, 0, 0, 0, 2))
BVH_CAPACITY, LEGACY_CAPACITY = 256 * 9, 256 * 10
MODULES = {
    "absent": dict(module=0, blocks_per_cu5=0, blocks_per_cu6=0, blocks_per_cu_bvh=0,
                   blocks_per_cu_legacy=0, has_legacy=0, has_bvh_path=0, has_bvh_primary=0),
    "complete": dict(module=1, blocks_per_cu5=11, blocks_per_cu6=12, blocks_per_cu_bvh=13,
                     blocks_per_cu_legacy=14, has_legacy=1, has_bvh_path=1, has_bvh_primary=1),
    "no_bvh": dict(module=1, blocks_per_cu5=11, blocks_per_cu6=12, blocks_per_cu_bvh=0,
                   blocks_per_cu_legacy=14, has_legacy=1, has_bvh_path=0, has_bvh_primary=0),
    "zero_blocks": dict(module=1, blocks_per_cu5=0, blocks_per_cu6=0, blocks_per_cu_bvh=0,
                        blocks_per_cu_legacy=0, has_legacy=1, has_bvh_path=1, has_bvh_primary=1),
}


@functools.lru_cache(maxsize=None)
def constants():
    """The constants of csrc/rvcp_internal.h the plan uses, by name."""
    text = open(INTERNAL_H).read()
    out = {}
    m = re.search(r"#define\s+RVCP_TILED_POOL_WAVES\s+(\d+)", text)
    assert m, "RVCP_TILED_POOL_WAVES not found in rvcp_internal.h"
    out["kTiledPoolWaves"] = int(m.group(1))
    for name in ("kWave", "kBlock", "kChunk", "kMinStatic", "kDefaultVariant", "kMaxVariant",
                 "kTiledPoolVariant", "kWideMinSamples", "kSpecWideMinSamples",
                 "kPrepassBatchMaxPixels", "kTiledDualMinSamples", "kTiledWideMinFaces",
                 "kTiledMinFaces"):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9uUlL\s*<]+);", text)
        assert m, name + " not found in rvcp_internal.h"
        expr = re.sub(r"(\d+)[uUlL]*", r"\1", m.group(1))       # "8ull << 20", "512u * 1024u", "64"
        if "<<" in expr:
            a, b = expr.split("<<")
            out[name] = int(a) << int(b)
        else:
            out[name] = 1
            for factor in expr.split("*"):
                out[name] *= int(factor)
    return out


def static_split(n, grid_waves, n_simds):
    """(waves, chunk): full kChunk-pixel waves unless that leaves fewer than two waves per SIMD;
    then up to two waves per SIMD, at least kMinStatic pixels each; never more than the grid."""
    K = constants()
    chunk_px, min_px = K["kChunk"], K["kMinStatic"]
    waves = max(-(-n // chunk_px), min(-(-n // min_px), 2 * n_simds))
    waves = max(1, min(waves, grid_waves))
    return waves, min(max(-(-n // waves), 1), chunk_px)


def make_input(module="absent", **kw):
    """A plan input: the test device's numbers, a module by name, the rest from kw."""
    inp = dict(integrator=abi.INTEGRATOR_GAMES101, kernel_variant=0, accel=abi.ACCEL_NONE, spp=1,
               max_bounces=5, attenuation_stop_eps=0.01, ray_t_min=1e-3, grid_waves_per_simd=0,
               n_faces=32, bvh_prefix=0, n_simds=N_SIMDS, grid_capacity=GRID_CAPACITY,
               bvh_capacity=BVH_CAPACITY, legacy_capacity=LEGACY_CAPACITY, n_frames=1, frame_px=0,
               stride=0, spread_min=0)
    inp.update(MODULES[module])
    inp.update(kw)
    assert set(inp) == set(FIELDS), set(inp) ^ set(FIELDS)
    return inp


def line(inp):
    """The input as tools/frame_plan_check.cpp reads it."""
    parts = []
    for f in FIELDS:
        v = inp[f]
        if f == "grid_capacity":
            parts.extend(str(int(c)) for c in v)
        elif f in ("attenuation_stop_eps", "ray_t_min"):
            parts.append(repr(float(v)))
        else:
            parts.append(str(int(v)))
    return " ".join(parts)


def plan(inp):
    """The plan of one input, by OUT_FIELDS."""
    K = constants()
    legacy = inp["integrator"] == abi.INTEGRATOR_LEGACY
    bvh = inp["accel"] == abi.ACCEL_BVH and inp["n_faces"] > 0
    module = bool(inp["module"])
    t_min_pos = inp["ray_t_min"] > 0.0
    px, n_frames = inp["frame_px"], inp["n_frames"]
    samples = px * inp["spp"]

    # the schedule: the BVH's kernels are schedule 3's; else the caller's; else by mesh and frame
    if bvh:
        variant = 3
    elif inp["kernel_variant"] != 0:
        variant = inp["kernel_variant"]
    else:
        spec_scan = module and t_min_pos
        big = samples >= K["kTiledDualMinSamples"]
        if inp["n_faces"] >= K["kTiledMinFaces"]:
            variant = K["kTiledPoolVariant"] if big else 5
        elif not spec_scan and inp["n_faces"] > K["kTiledWideMinFaces"] and big:
            variant = K["kTiledPoolVariant"]
        elif samples >= (K["kSpecWideMinSamples"] if spec_scan else K["kWideMinSamples"]):
            variant = 6
        else:
            variant = K["kDefaultVariant"]

    trivial = inp["max_bounces"] == 0 or (not legacy and inp["attenuation_stop_eps"] > 1.0)
    P = dict.fromkeys(OUT_FIELDS, 0)
    P.update(status=abi.RVCP_OK, variant=variant, accel=abi.ACCEL_BVH if bvh else abi.ACCEL_NONE,
             trivial=int(trivial), legacy=int(legacy))
    if n_frames > 1 and not trivial and not legacy and variant < 3:
        P["status"] = abi.RVCP_E_UNSUPPORTED
        return P
    cams = n_frames > 1 and not trivial and px > 0 and (legacy or variant >= 3)
    P.update(cams=int(cams), prepass_batched=int(cams and px <= K["kPrepassBatchMaxPixels"]),
             out_px=n_frames * inp["stride"] if n_frames > 1 else px)
    if trivial or px == 0:
        return P

    # which of the module's kernels run, and the resident workgroups of the kernel that does
    per_cu = 0
    spec = spec_bvh = spec_legacy = False
    if legacy:
        cap = inp["legacy_capacity"]
        if module and inp["has_legacy"] and inp["blocks_per_cu_legacy"] > 0:
            spec_legacy, per_cu = True, inp["blocks_per_cu_legacy"]
    elif bvh:
        cap = inp["bvh_capacity"]
        if (module and inp["bvh_prefix"] > 0 and inp["has_bvh_path"] and inp["has_bvh_primary"]
                and inp["blocks_per_cu_bvh"] > 0 and t_min_pos):
            spec_bvh, per_cu = True, inp["blocks_per_cu_bvh"]
    else:
        cap = inp["grid_capacity"][variant]
        n = {3: inp["blocks_per_cu5"], 6: inp["blocks_per_cu6"]}.get(variant, 0)
        if module and n > 0 and t_min_pos:
            spec, per_cu = True, n
    if per_cu:
        cap = per_cu * (inp["n_simds"] // 4)
    pool = not legacy and not bvh and variant == K["kTiledPoolVariant"]
    wpb = K["kTiledPoolWaves"] if pool else K["kBlock"] // K["kWave"]
    if inp["grid_waves_per_simd"] > 0:
        cap = min(cap, max(1, inp["grid_waves_per_simd"] * inp["n_simds"] // wpb))
    waves, chunk = static_split(px * n_frames, cap * wpb, inp["n_simds"])
    blocks = max(1, min(-(-waves // wpb), cap))
    if inp["spread_min"] and not legacy and not bvh and variant in (3, 6):
        blocks = cap
    code = 8 if legacy else 7 if bvh else variant
    if spec or spec_bvh or spec_legacy:
        code |= abi.VARIANT_SPECIALIZED
    P.update(spec=int(spec), spec_bvh=int(spec_bvh), spec_legacy=int(spec_legacy), cap=cap, wpb=wpb,
             blocks=blocks, static_chunk=chunk, static_chunks=waves * chunk, stats_code=code)
    return P
