"""G-buffer render and a-trous denoiser on the GPU: every texel and every
filtered float bit-identical to the CPU restatements (tests/denoise_ref.py: the oracle's primary
ray + pyref's triangle test for the G-buffer, the numpy float32 filter for the denoiser), the
RGBA8 store equal to oracle.gamma_u8 of those floats, the filter's exact invariants, the
end-to-end chain with its quality gate, and the argument checks.  Every rejected call is
rejected on the host before any launch."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R
import oracle as O
import rvcp_amd
from rvcp_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    """A numpy array's bytes in a torch device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.fixture(scope="module")
def tracers():
    """One scene-less context per unorm_rule: the denoiser needs no scene."""
    rts = [rvcp_amd.RayTracer(unorm_rule=rule) for rule in (abi.UNORM_DRIVER, abi.UNORM_NEAREST)]
    yield rts
    for rt in rts:
        rt.close()


def gpu_gbuffer(rt, sc, W, H):
    out = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.render_gbuffer_async(sc.push_constant(0.0), W, H, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W)


def gpu_denoise(rt, c, g, params, want_rgba=True):
    """rvcp_denoise_async on device tensors (the context's own stream); (floats, rgba)."""
    H, W = c.shape[:2]
    d_in, d_g = dev(c), dev(g)
    d_out = torch.zeros(W * H * 12, dtype=torch.uint8, device="cuda")
    d_rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rt.denoise_async(d_in.data_ptr(), d_g.data_ptr(), W, H, d_out.data_ptr(),
                     d_rgba.data_ptr() if want_rgba else 0, params)
    assert rt.denoise_wait() >= 0.0
    return (d_out.cpu().numpy().view(np.float32).reshape(H, W, 3),
            d_rgba.cpu().numpy().reshape(H, W, 4))


# ---------------------------------------------------------------------------- 1. G-buffer
@pytest.mark.parametrize("rotated", [False, True])
def test_gbuffer_matches_cpu_scan(rotated):
    W, H = 37, 23
    ref = R.cornell_gbuffer(W, H, rotated)
    miss = ref["face"] == R.MISS
    emis = (ref["material"] & np.uint32(R.EMISSIVE)) != 0
    assert miss.any() and emis.any() and R.filterable(ref).any()
    assert not ref["position"][miss].any() and not ref["normal"][miss].any()
    sc = rvcp_amd.Scene.default()
    if rotated:
        sc = rvcp_amd.scene.rotated_scene(sc)
    with rvcp_amd.RayTracer(spp=1) as rt:
        rt.upload_scene(sc)
        got = gpu_gbuffer(rt, sc, W, H)
    bad = [(y, x) for y in range(H) for x in range(W) if got[y, x].tobytes() != ref[y, x].tobytes()]
    assert not bad, f"{len(bad)} texels differ, first {bad[0]}: {got[bad[0]]} != {ref[bad[0]]}"


def test_gbuffer_bvh_equals_brute_force(cornell):
    sc = rvcp_amd.scene.with_random_triangles(cornell, 2000)
    W = H = 40
    res = []
    for accel in (abi.ACCEL_NONE, abi.ACCEL_BVH):
        with rvcp_amd.RayTracer(spp=1, accel=accel) as rt:
            rt.upload_scene(sc)
            res.append(gpu_gbuffer(rt, sc, W, H))
    f = res[0]["face"]
    assert ((f >= 32) & (f != R.MISS)).any() and (f < 32).any()    # random triangles and walls
    assert res[0].tobytes() == res[1].tobytes()


# ---------------------------------------------------------------------------- 2. denoise parity
CASES = [  # W, H, params
    (67, 45, dict(iterations=5, normal_power_log2=5, sigma_color=1.0, sigma_plane=1.0)),
    (67, 45, dict(iterations=3, normal_power_log2=8, sigma_color=float("inf"), sigma_plane=30.0)),
    (67, 45, dict(iterations=8, normal_power_log2=0, sigma_color=300.0, sigma_plane=5.0)),
    (130, 3, dict(iterations=5, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
    (8, 8, dict(iterations=1, normal_power_log2=1, sigma_color=0.3, sigma_plane=10.0)),
    (8, 8, dict(iterations=8, normal_power_log2=3, sigma_color=float("inf"), sigma_plane=1.0)),
    (1, 1, dict(iterations=3, normal_power_log2=5, sigma_color=1.0, sigma_plane=1.0)),
    # the reach of the passes: at eight passes the steps 32, 64 and 128 have taps inside the frame
    # at both distances, along a row and along a column
    (261, 5, dict(iterations=8, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
    (5, 261, dict(iterations=8, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
    # frames exactly on and one past the 32 x 8 and the 64 x 4 tiles
    (64, 8, dict(iterations=5, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
    (65, 9, dict(iterations=5, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
    (33, 5, dict(iterations=5, normal_power_log2=2, sigma_color=50.0, sigma_plane=100.0)),
]


@pytest.mark.parametrize("W,H,kw", CASES)
def test_denoise_matches_numpy_restatement(tracers, W, H, kw):
    c, g = R.synthetic_case(W, H, seed=W * 1000 + H)
    if W * H > 1:
        assert R.filterable(g).any() and not R.filterable(g).all()
    else:
        g["face"], g["material"] = 7, 2              # the single pixel is filterable
    params = abi.make_denoise_params(**kw)
    want = R.denoise_params(c, g, params)
    for rule, rt in enumerate(tracers):
        got, rgba = gpu_denoise(rt, c, g, params)
        diff = np.any(bits(got) != bits(want), axis=-1)
        assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ (rule {rule})"
        assert np.array_equal(rgba, R.gamma_rgba(want, rule)), rule


def test_denoise_default_params_and_no_rgba(tracers):
    """params = NULL takes rvcp_denoise_params_default; d_rgba8_out is optional."""
    c, g = R.synthetic_case(33, 17, seed=11, color_max=4.0)
    want = R.denoise_params(c, g, abi.make_denoise_params())
    got, rgba = gpu_denoise(tracers[0], c, g, None, want_rgba=False)
    assert np.array_equal(bits(got), bits(want))
    assert not rgba.any()


# ---------------------------------------------------------------------------- 3. exact invariants
KW = dict(iterations=5, normal_power_log2=0, sigma_color=float("inf"), sigma_plane=0.25)


def test_gpu_half_planes_do_not_mix(tracers):
    c, g, left = R.half_planes()
    out, _ = gpu_denoise(tracers[0], c, g, abi.make_denoise_params(**KW))
    assert np.all(bits(out[left]) == bits(np.float32(0.0)))
    assert np.all(bits(out[~left]) == bits(np.float32(1.0)))


def test_gpu_non_filterable_pixels_pass_through_and_feed_nothing(tracers):
    c, g = R.synthetic_case(45, 31, seed=3)
    filt = R.filterable(g)
    p = abi.make_denoise_params(iterations=3, normal_power_log2=5, sigma_color=1.0, sigma_plane=1.0)
    out, _ = gpu_denoise(tracers[0], c, g, p)
    assert np.array_equal(bits(out[~filt]), bits(c[~filt]))
    hot = c.copy()
    hot[~filt] = 1.0e30
    out_hot, _ = gpu_denoise(tracers[0], hot, g, p)
    assert np.array_equal(bits(out_hot[filt]), bits(out[filt]))
    assert np.array_equal(bits(out_hot[~filt]), bits(hot[~filt]))


def test_gpu_partition_of_unity(tracers):
    c, g = R.coplanar_patch()
    out, _ = gpu_denoise(tracers[0], c, g, abi.make_denoise_params(**KW))
    assert np.all(np.abs(out.astype(np.float64) / c.astype(np.float64) - 1.0) <= 1e-5)


# ---------------------------------------------------------------------------- 4. end to end
def test_render_denoised_end_to_end(cornell, cornell_arrays):
    """render_denoised at 64^2 SPP = 4 == oracle linear -> CPU G-buffer -> numpy filter ->
    gamma_u8, bytes and floats; and the quality gate of the CPU test on the GPU's frame."""
    W = H = 64
    params = abi.make_denoise_params()
    with rvcp_amd.RayTracer(spp=4) as rt:
        rt.upload_scene(cornell)
        rgba, lin = rt.render_denoised(W, H, 5.0, params, want_linear=True)
        assert rt.last_denoise_ms > 0.0 and int(rt.last_stats["samples"]) == W * H * 4
        raw = rt.render(W, H, 5.0)                       # the plain call still works afterwards
    noisy, o_rgba, _ = O.render(cornell_arrays, cornell.push_constant(5.0),
                                abi.make_config(spp=4), W, H)
    assert np.array_equal(raw, o_rgba)
    g = R.cornell_gbuffer(W, H)
    want = R.denoise_params(noisy, g, params)
    assert np.array_equal(bits(lin), bits(want))
    assert np.array_equal(rgba, R.gamma_rgba(want))
    mask, ref = R.filterable(g), R.cornell_reference(W, H)
    before, after = R.rmse(noisy, ref, mask), R.rmse(lin, ref, mask)
    print(f"rmse noisy {before:.4f} denoised {after:.4f} ratio {after / before:.4f}")
    assert after <= R.QUALITY_GATE * before


# ---------------------------------------------------------------------------- 5. API
def test_api_argument_checks(cornell, cornell_arrays):
    L = abi.load()
    W = H = 16
    c, g = R.synthetic_case(W, H, seed=5, color_max=2.0)
    d_in, d_g = dev(c), dev(g)
    d_out = torch.zeros(W * H * 12 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P = ctypes.c_void_p
    push = np.ascontiguousarray(cornell.push_constant(1.0))
    with rvcp_amd.RayTracer(spp=2) as rt:                # no scene uploaded
        h = rt.handle

        def denoise(inp, gb, w, hh, params, out):
            return L.rvcp_denoise_async(h, P(inp) if inp else None, P(gb) if gb else None, w, hh,
                                        abi.ptr(params), P(out) if out else None, None, None)
        ok = abi.make_denoise_params(iterations=2)
        a, b, o = d_in.data_ptr(), d_g.data_ptr(), d_out.data_ptr()
        E = abi.RVCP_E_INVALID
        assert denoise(0, b, W, H, ok, o) == E
        assert denoise(a, 0, W, H, ok, o) == E
        assert denoise(a, b, W, H, ok, 0) == E
        assert denoise(a, b, 0, H, ok, o) == E and denoise(a, b, W, 0, ok, o) == E
        assert denoise(a, b, W, H, abi.make_denoise_params(iterations=0), o) == E
        assert denoise(a, b, W, H, abi.make_denoise_params(iterations=9), o) == E
        assert denoise(a, b, W, H, abi.make_denoise_params(normal_power_log2=9), o) == E
        assert denoise(a, b, W, H, abi.make_denoise_params(sigma_color=0.0), o) == E
        assert denoise(a, b, W, H, abi.make_denoise_params(sigma_plane=float("nan")), o) == E
        assert denoise(a, b, W, H, ok, a) == E                  # output aliases the input
        assert denoise(a, b, W, H, ok, a + 12) == E             # ... or overlaps it
        assert b"overlap" in L.rvcp_last_error(h)
        assert L.rvcp_denoise_wait(h, None) == E                # nothing was enqueued
        # the G-buffer needs a scene; the denoiser does not
        assert L.rvcp_render_gbuffer_async(h, abi.ptr(push), W, H, P(o), None) == abi.RVCP_E_NO_SCENE
        assert L.rvcp_render_gbuffer_async(h, None, W, H, P(o), None) == E
        assert L.rvcp_render_gbuffer_async(h, abi.ptr(push), W, H, None, None) == E
        assert L.rvcp_render_gbuffer_async(h, abi.ptr(push), 0, H, P(o), None) == E
        assert denoise(a, b, W, H, ok, o) == abi.RVCP_OK
        assert rt.denoise_wait() >= 0.0
        got = d_out.cpu().numpy()[:W * H * 12].view(np.float32).reshape(H, W, 3)
        assert np.array_equal(bits(got), bits(R.denoise_params(c, g, ok)))
        # after all of that a plain render is still bit-exact against the oracle
        rt.upload_scene(cornell)
        rgba, lin = rt.render(32, 32, 123.0, want_linear=True)
    o_lin, o_rgba, _ = O.render(cornell_arrays, cornell.push_constant(123.0),
                                abi.make_config(spp=2), 32, 32)
    assert np.array_equal(rgba, o_rgba) and np.array_equal(bits(lin), bits(o_lin))


@pytest.mark.parametrize("kw", [dict(integrator=abi.INTEGRATOR_LEGACY), dict(n_gpus=2)])
def test_gbuffer_unsupported_contexts(cornell, kw):
    d = torch.zeros(16 * 16 * 32, dtype=torch.uint8, device="cuda")
    with rvcp_amd.RayTracer(**kw) as rt:
        rt.upload_scene(cornell)
        with pytest.raises(abi.RvcpError) as e:
            rt.render_gbuffer_async(cornell.push_constant(1.0), 16, 16, d.data_ptr())
        assert e.value.code == abi.RVCP_E_UNSUPPORTED
        with pytest.raises(abi.RvcpError) as e:
            rt.render_denoised(16, 16, 1.0)
        assert e.value.code == abi.RVCP_E_UNSUPPORTED


def test_bad_filter_parameters_midway_leave_nothing_pending(cornell):
    """render_denoised whose filter is rejected after the render was enqueued leaves neither a
    frame nor a filter pending, and the context goes on as before."""
    L = abi.load()
    W = H = 16
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        raw = rt.render(W, H, 1.0)
        good = rt.render_denoised(W, H, 2.0, want_linear=True)
        with pytest.raises(abi.RvcpError) as e:
            rt.render_denoised(W, H, 3.0, abi.make_denoise_params(iterations=9))
        assert e.value.code == abi.RVCP_E_INVALID and "denoise iterations" in str(e.value)
        assert L.rvcp_denoise_wait(rt.handle, None) == abi.RVCP_E_INVALID
        assert b"in flight" in L.rvcp_last_error(rt.handle)
        assert np.array_equal(rt.render(W, H, 1.0), raw)
        again = rt.render_denoised(W, H, 2.0, want_linear=True)
    assert np.array_equal(again[0], good[0]) and np.array_equal(bits(again[1]), bits(good[1]))


def test_denoise_is_ordered_behind_a_pending_render(cornell, cornell_arrays):
    """A render pending on the context is no error for the denoiser: on the same stream the
    filter reads the frame that render leaves."""
    W = H = 24
    params = abi.make_denoise_params(iterations=2)
    d_rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    d_lin = torch.zeros(W * H * 12, dtype=torch.uint8, device="cuda")
    d_g = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(W * H * 12, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    push = cornell.push_constant(9.0)
    with rvcp_amd.RayTracer(spp=2) as rt:
        rt.upload_scene(cornell)
        rt.render_async(push, W, H, d_rgba.data_ptr(), d_lin.data_ptr())
        rt.render_gbuffer_async(push, W, H, d_g.data_ptr())
        rt.denoise_async(d_lin.data_ptr(), d_g.data_ptr(), W, H, d_out.data_ptr(), params=params)
        rt.wait()
        rt.denoise_wait()
    noisy, _, _ = O.render(cornell_arrays, push, abi.make_config(spp=2), W, H)
    g = d_g.cpu().numpy().view(abi.GBUFFER_DTYPE).reshape(H, W)
    want = R.denoise_params(noisy, g, params)
    assert np.array_equal(bits(d_out.cpu().numpy().view(np.float32).reshape(H, W, 3)), bits(want))
