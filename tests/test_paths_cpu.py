"""Path queries without a GPU: the exported symbols, and the reference of
tests/paths_ref.py pinned to the oracle -- on a frame's own rays (oracle.sample_ray) and seeds it
gives oracle.render's linear frame bit for bit and, summed over the frame, the oracle's traversal
count; and its two own rules (a non-finite ray, a seed outside [0, 1): zeros, no traversal)."""
import subprocess

import numpy as np
import pytest

import oracle
import paths_ref
from conftest import scene_arrays
from rvcp_amd import abi

f32 = np.float32
W, H = 12, 8
SYMBOLS = ("rvcp_trace_paths_async", "rvcp_paths_wait", "rvcp_trace_paths",
           "rvcp_primary_seeds_async")


def test_library_exports_the_four_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported
    assert set(SYMBOLS) <= set(abi.EXPORTED)
    L = abi.load()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None
    assert L.rvcp_abi_version() == abi.ABI_VERSION == 2


def test_null_context_is_invalid():
    L = abi.load()
    p = abi.ptr(np.zeros(64, np.uint8))
    assert L.rvcp_trace_paths_async(None, p, p, 1, 1, p, None) == abi.RVCP_E_INVALID
    assert L.rvcp_paths_wait(None, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_trace_paths(None, p, p, 1, 1, p, None, None) == abi.RVCP_E_INVALID
    assert L.rvcp_primary_seeds_async(None, p, 4, 4, p, None) == abi.RVCP_E_INVALID


def frame_rays(push):
    rows = [oracle.sample_ray(push, W, H, x, y) for y in range(H) for x in range(W)]
    return np.ascontiguousarray(np.array(rows, f32)).view(paths_ref.RAY_DTYPE).reshape(-1)


@pytest.mark.parametrize("spp", [2, 3])
def test_reference_on_a_frames_rays_is_the_oracles_frame(cornell, spp):
    cfg = abi.make_config(spp=spp)
    push = cornell.push_constant(3.0)
    want, _, want_trav = oracle.render(scene_arrays(cornell), push, cfg, W, H)
    seeds = paths_ref.frame_seeds(push["time"], W, H)
    assert ((seeds >= 0) & (seeds < 1)).all()
    lin, trav = paths_ref.trace_paths(cornell, cfg, frame_rays(push), seeds, spp)
    assert np.array_equal(lin.view(np.uint32), want.reshape(-1, 3).view(np.uint32))
    assert int(trav.sum()) == want_trav
    # the frame has pixels of every kind: surfaces (more traversals than samples), and first hits
    # that end the sample at once (the light, or a miss: one traversal per sample)
    assert (trav > spp).any() and (trav == spp).any()


def test_zero_rules(cornell):
    cfg = abi.make_config(spp=2)
    push = cornell.push_constant(0.0)
    good = frame_rays(push)[W * (H // 2) + W // 2: W * (H // 2) + W // 2 + 1]
    lin, trav = paths_ref.trace_paths(cornell, cfg, good, [0.25], 2)
    assert trav[0] > 0 and (lin != 0).any()
    flat = good.view(f32).reshape(-1)
    for k in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = flat.copy()
            r[k] = bad
            lin, trav = paths_ref.trace_paths(cornell, cfg, r.view(paths_ref.RAY_DTYPE), [0.25], 2)
            assert trav[0] == 0 and not lin.any(), (k, bad)
    for seed in (np.nan, -0.25, 1.0, np.inf, -np.inf, 1.5):
        lin, trav = paths_ref.trace_paths(cornell, cfg, good, [seed], 2)
        assert trav[0] == 0 and not lin.any(), seed
    for seed in (0.0, np.nextafter(f32(1.0), f32(0.0))):          # the ends of [0, 1)
        lin, trav = paths_ref.trace_paths(cornell, cfg, good, [seed], 2)
        assert trav[0] > 0, seed
