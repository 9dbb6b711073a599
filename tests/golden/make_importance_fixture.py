"""Generate tests/golden/importance_frames.npz: small frames of the cosine-weighted bounce
(RVCP_SAMPLING_COSINE) rendered by its pure-Python restatement,
tests/importance_ref.py -- the mode has no C oracle, so these committed frames are what the HIP
kernels are compared with, bit for bit (tests/test_gpu_importance.py), and what pins the
restatement itself (tests/test_importance_cpu.py).

Cases (importance_ref.CASES, all at time importance_ref.FIXTURE_TIME): the default Cornell box at
16 x 16 SPP = 3, scene.rotated_scene of it at 12 x 12 SPP = 2, and two fuzz scenes of
tests/fuzz_scenes.py at 12 x 10 with their own configs.  Each stores the linear RGB (float32),
the RGBA8 frame (oracle.gamma_u8 of it), the traversal count per pixel and in total, and the
SHA-256 of the scene buffers.  About a minute.

  python tests/golden/make_importance_fixture.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import denoise_ref  # noqa: E402
import importance_ref as I  # noqa: E402
import rvcp_amd  # noqa: E402

OUT = os.path.join(HERE, "importance_frames.npz")


def scene_digest(sc):
    h = hashlib.sha256()
    for a in (sc.aligned_materials(), sc.mesh.aligned_vertices(), sc.mesh.aligned_faces(),
              sc.luminous_face_ids()):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    out = {}
    for case in I.CASES:
        sc, kw, W, H = I.case_scene(case)
        cfg = rvcp_amd.abi.make_config(**kw)
        lin, trav = I.render(sc, cfg, sc.push_constant(I.FIXTURE_TIME), W, H)
        out[case + "/linear"] = lin
        out[case + "/rgba"] = denoise_ref.gamma_rgba(lin)
        out[case + "/traversals_px"] = trav
        out[case + "/traversals"] = np.array(int(trav.sum(dtype=np.uint64)), dtype=np.uint64)
        out[case + "/scene_sha256"] = np.array(scene_digest(sc))
        print(case, lin.shape, int(trav.sum()), "samples", W * H * int(cfg["spp"]),
              scene_digest(sc)[:16], flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
