"""devmath -- ctypes loader of the device-primitive harness (tests/devmath/rvcp_devmath.hip, built
by `make -C csrc devmath` / __graft_entry__.build() into csrc/build/librvcp_devmath.so).
TEST INFRASTRUCTURE ONLY: the package never loads this library.  A missing library is an error,
never a skip.  RVCP_DEVMATH_LIB selects another build of the harness (scratch builds with one
primitive changed: how the mutation table of tests/test_gpu_devmath.py was made)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "rvcp-real-time-path-tracer_amd", "csrc", "build", "librvcp_devmath.so")

# op: (number, input words per record, output words per record or None when it depends on draws)
OPS = {
    "sqrt": (0, 1, 1), "rcp_ieee": (1, 1, 1), "rcp_scan": (2, 1, 1), "rcp_scan_fast": (3, 1, 1),
    "normalize": (4, 3, 3), "divs_y": (5, 4, 3), "divs_pos": (6, 4, 3), "markstein": (7, 2, 1),
    "sphere": (8, 12, 4), "sinf": (9, 1, 1), "sinf_rand": (10, 1, 1), "rand_of": (11, 1, 1),
    "rnd_stream": (12, 2, None), "pixel_seed": (13, 3, None), "tri": (14, 26, 11),
    "shadow_stop": (15, 6, 1), "cosine_bounce": (16, 12, 6), "pack_rgb8": (17, 3, 1),
}
_lib = None
_failed = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("RVCP_DEVMATH_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(f"the device-primitive harness {path} is not built: run "
                               "__graft_entry__.build() (or make -C csrc devmath)")
        L = ctypes.CDLL(path)
        L.rvcp_devmath_eval.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p]
        L.rvcp_devmath_eval.restype = ctypes.c_int
        _lib = L
    return _lib


def run(op: str, records, params=None) -> np.ndarray:
    """Run `op` over `records` ([n, in words] or [n] float32 / uint32) on cuda:0: upload, one
    harness call, synchronise.  Returns the output records as uint32 [n, out words]."""
    import torch
    num, win, wout = OPS[op]
    L = lib()
    a = np.ascontiguousarray(records)
    assert a.dtype in (np.float32, np.uint32), a.dtype
    a = a.view(np.int32).reshape(-1, win)
    n = len(a)
    par = None if params is None else np.ascontiguousarray(params, dtype=np.float32)
    if wout is None:
        wout = int(par[0]) + 1
    global _failed
    if _failed:
        raise RuntimeError(f"not run: an earlier harness call failed on the device ({_failed})")
    try:
        d_in = torch.from_numpy(a).to("cuda:0")
        d_out = torch.zeros((n, wout), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        rc = L.rvcp_devmath_eval(num, d_in.data_ptr(), d_out.data_ptr(), n,
                                 None if par is None else par.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError(f"rvcp_devmath_eval({op}) failed: {rc}")
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(np.uint32)
    except Exception as e:
        _failed = f"{op}: {e}"       # a device error is sticky: launch nothing after it
        raise
