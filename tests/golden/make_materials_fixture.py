"""Generate tests/golden/materials_frames.npz: small frames of the material scattering mode
(RVCP_MATERIALS_SCATTER) rendered by its pure-Python restatement,
tests/materials_ref.py -- the mode has no C oracle, so these committed frames are what the HIP
kernel is compared with, bit for bit (tests/test_gpu_materials.py), and what pins the restatement
itself (tests/test_materials_cpu.py).

Cases (materials_ref.CASES, all at time materials_ref.FIXTURE_TIME): scene.specular_cornell_scene
at 24 x 16 SPP = 2 with the default configuration, with fuzz = 0.3, without the light-pick quirk
and with max_bounces = 3, rr = 1; a box of fuzz-1 metal walls at 16 x 12 SPP = 1.  Each stores the
linear RGB (float32), the RGBA8 frame (oracle.gamma_u8 of it), the traversal count per pixel and in
total and the restatement's event counters.  `mirror/*` is the mirror test: 1024 rays straight down
onto the mirror floor.  Well under a minute.

  python tests/golden/make_materials_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import denoise_ref  # noqa: E402
import materials_ref as M  # noqa: E402

OUT = os.path.join(HERE, "materials_frames.npz")


def main():
    out = {}
    for case in M.CASES:
        ev = M.new_events()
        lin, trav = M.case_frame(case, ev)
        out[case + "/linear"] = lin
        out[case + "/rgba"] = denoise_ref.gamma_rgba(lin)
        out[case + "/traversals_px"] = trav
        out[case + "/traversals"] = np.array(int(trav.sum(dtype=np.uint64)), dtype=np.uint64)
        out[case + "/events"] = np.array([ev[k] for k in M.EVENTS], dtype=np.uint64)
        print(case, lin.shape, int(trav.sum()), ev, flush=True)
    lin, trav = M.mirror_result()
    out["mirror/linear"] = lin
    out["mirror/traversals"] = trav
    print("mirror", int(np.count_nonzero(lin.any(axis=1))), "of", len(lin), "survive", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
