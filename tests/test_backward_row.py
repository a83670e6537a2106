"""The backward row: frames with plain SH colours leave ten floats per Gaussian (nine direction terms T[ch][axis] = sum_k dB_k/d axis * sh[k][ch] and
the combined opacity) for the per-Gaussian backward kernel, which then reads neither the SH block nor the splat record and recomputes the 3-D
covariance from scales and rotations (csrc/wg_common.h: bwd_row_terms, cov3d_from_scale_rot; include/wg_rasterizer.h: wg_forward_args::forward_only).

Gradients are held to the CPU oracle with the bound tests/test_parity_gpu.py applies to the same tensors (1e-3 max-rel-err per tensor); route
against route the bits are compared under deterministic_backward = 1.  Scenes are 64x48 and at most 130 Gaussians, but for the lazy-colour case,
which needs the dense frame of test_lazy_colour_of_split_frames_changes_no_result to make the split happen at all."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import wg_scenes as S
from wg_testlib import compare_grads, make_settings, run_hip, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))   # the compiled binding
GRAD_BOUND = 1e-3   # tests/test_parity_gpu.py: gradients <= 1e-3 max-rel-err per tensor
W, H = 64, 48
ROW_FLOATS = 10


def _scene(P, deg, M=16, seed=3):
    """P Gaussians over the 64x48 frame, SH degree `deg` stored with M coefficients (the unused ones random: they must not matter).  From 63
    Gaussians on: three behind the camera, two each with one / two / three colour channels driven negative (clamp flags 1, 3, 7), eight opaque
    covers in front of the frame's centre and four Gaussians behind them that are visible but blend nowhere."""
    cloud = S.make_cloud(P, W, H, sh_degree=deg, seed=seed, scale_mult=25.0)
    rng = np.random.default_rng(100 + seed)
    sh = rng.normal(0.0, 0.1, size=(P, M, 3)).astype(np.float32)
    sh[:, :(deg + 1) ** 2] = cloud["shs"]
    if P >= 63:
        m, sc, op = cloud["means3D"], cloud["scales"], cloud["opacities"]
        m[3:6, 2] = -1.0
        m[6:12, :2] *= 0.5          # (well inside the frame)
        sh[6:12, 0, :] = 1.0
        sh[6:8, 0, 0] = -3.0
        sh[8:10, 0, :2] = -3.0
        sh[10:12, 0, :] = -3.0
        for j, i in enumerate(range(12, 20)):
            m[i] = (0.0, 0.0, 0.8 + 0.01 * j)
            sc[i] = 0.12
            op[i] = 0.99
        for j, i in enumerate(range(20, 24)):
            m[i] = (0.05 * j - 0.1, 0.02 * j, 6.0)
            sc[i] = 0.05
    cloud["shs"] = sh
    return cloud


def _native(cloud, cam, deg, cot, forward_only=False, raw=None, **opts):
    """Forward and backward through the native module, keeping the buffers -> dict(color, radii, views, grads as numpy by wg_testlib.GRAD_NAMES)."""
    from diff_gaussian_rasterization import _C
    rs = make_settings(cam, deg)
    e = torch.Tensor([])
    t = {k: to_dev(v) for k, v in cloud.items()}
    P = t["means3D"].shape[0]
    args = (rs.bg, t["means3D"], t.get("colors_precomp", e), t["opacities"], t.get("scales", e), t.get("rotations", e), 1.0, t.get("cov3D_precomp", e),
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width,
            t.get("shs", e), deg, rs.campos, False, False)
    extra = {} if raw is None else {"filter_3D": to_dev(raw)}
    R, color, radii, gb, bb, ib = _C.rasterize_gaussians(*args, forward_only=forward_only, options=opts or None, **extra)
    out = dict(color=color, radii=radii, geometry=_C.view_geometry(gb, P), image=_C.view_image(ib, rs.image_height, rs.image_width), R=R)
    if cot is not None:
        g = _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, t.get("colors_precomp", e), t.get("scales", e), t.get("rotations", e), 1.0,
                                            t.get("cov3D_precomp", e), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size,
                                            rs.subpixel_offset, to_dev(cot), t.get("shs", e), deg, rs.campos, gb, R, bb, ib, False, options=opts or None,
                                            **({} if raw is None else {"raw": (to_dev(raw), t["opacities"])}))
        names = ("means2D", "colors_precomp", "opacities", "means3D", "cov3Ds_precomp", "sh", "scales", "rotations")
        out["grads_t"] = dict(zip(names, g[:8]))
        out["grads"] = {k: v.cpu().numpy() for k, v in out["grads_t"].items() if k != "colors_precomp" or "colors_precomp" in cloud}
    return out


def _counters():
    from diff_gaussian_rasterization import _C
    return _C.get_option("backward_row_frames"), _C.get_option("backward_row_calls")


def _check_against_oracle(h_grads, o, what):
    errs = compare_grads(h_grads, o["grads"])
    print(what, errs)
    for k, e in errs.items():
        assert e <= GRAD_BOUND, (what, k, e, errs)
    return errs


# 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,deg,M", [(1, 3, 16), (63, 3, 16), (64, 0, 16), (65, 1, 16), (130, 2, 16), (130, 3, 16), (65, 2, 9), (130, 2, 9)])
def test_row_backward_matches_the_oracle(oracle, P, deg, M):
    """Partial and multiple 64-blocks, every SH degree in the 16-coefficient layout and degree 2 in the generic one (M = 9), through the autograd
    layer (which asks for the row: the inputs require gradients).  Culled Gaussians, clamp flags on one / two / three channels, covered Gaussians."""
    cam, cloud, cot = S.make_camera(W, H), _scene(P, deg, M), S.make_cotangent(W, H)
    f0, b0 = _counters()
    h = run_hip(cloud, cam, sh_degree=deg, cotangent=cot)
    f1, b1 = _counters()
    assert (f1 - f0, b1 - b0) == (1, 1)       # the frame left rows and its backward call ran on them
    o = oracle.run_scene(cloud, cam, sh_degree=deg, cotangent=cot)
    assert (h["radii"] == o["radii"]).all()
    _check_against_oracle(h["grads"], o, f"P={P} deg={deg} M={M}")
    culled = h["radii"] == 0
    assert not h["grads"]["sh"][culled].any()
    if P >= 63:
        assert culled[3:6].all() and (h["radii"][6:24] > 0).all()
        n = _native(cloud, cam, deg, None)
        assert n["geometry"]["clamped"][6:12].tolist() == [1, 1, 3, 3, 7, 7]
        assert not n["geometry"]["bwd_row"][to_dev(culled)].any()      # zero rows for culled Gaussians
        assert not h["grads"]["sh"][20:24].any()                          # covered: visible, blended nowhere
        assert np.isfinite(h["grads"]["means3D"]).all()


# 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_both_backward_paths_match_the_oracle_and_the_forward_is_the_same(oracle):
    """forward_only = 1 is a hint: the frame leaves no row, its backward call takes the kernel that re-reads the SH block, and both are right.
    Image, radii, n_contrib and final_T are the same bits either way."""
    cam, cloud, cot = S.make_camera(W, H), _scene(130, 3), S.make_cotangent(W, H)
    f0, b0 = _counters()
    a = _native(cloud, cam, 3, cot, forward_only=False)
    f1, b1 = _counters()
    b = _native(cloud, cam, 3, cot, forward_only=True)
    f2, b2 = _counters()
    assert (f1 - f0, b1 - b0, f2 - f1, b2 - b1) == (1, 1, 0, 0)
    assert a["geometry"]["bwd_row"] is not None and b["geometry"]["bwd_row"] is None     # (the forward_only frame's buffer holds no row array)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["radii"], b["radii"])
    for k in ("n_contrib", "final_T"):
        assert torch.equal(a["image"][k], b["image"][k]), k
    o = oracle.run_scene(cloud, cam, sh_degree=3, cotangent=cot)
    _check_against_oracle(a["grads"], o, "row path")
    _check_against_oracle(b["grads"], o, "SH re-read path")


# 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_routes_give_the_same_gradient_bits():
    """deterministic_backward = 1: every gradient is the same bits with the SH block streamed non-temporally or not.  The same data through the
    generic layout (an SH tensor that is not 16-byte aligned takes it; the suite has no option for it) gives the same rows and the same dL_dsh."""
    from diff_gaussian_rasterization import _C
    cam, cloud, cot = S.make_camera(W, H), _scene(130, 3), S.make_cotangent(W, H)
    outs = {}
    try:
        for st in (0, 1):
            _C.set_option("sh_stream", st)
            outs[st] = _native(cloud, cam, 3, cot, deterministic_backward=1)
    finally:
        _C.set_option("sh_stream", -1)
    for k, v in outs[0]["grads_t"].items():
        assert torch.equal(v, outs[1]["grads_t"][k]), k
    # the generic layout: the same coefficients at an address that is 4 modulo 16
    from diff_gaussian_rasterization import _C as C_
    rs = make_settings(cam, 3)
    t = {k: to_dev(v) for k, v in cloud.items()}
    P = t["means3D"].shape[0]
    store = torch.empty(P * 48 + 4, dtype=torch.float32, device="cuda")
    off = (1 - store.data_ptr() // 4) % 4          # element offset that makes the view's address = 4 (mod 16)
    sh_un = store[off:off + P * 48].view(P, 16, 3)
    sh_un.copy_(t["shs"])
    assert sh_un.data_ptr() % 16 == 4 and sh_un.is_contiguous()
    e = torch.Tensor([])
    f0, b0 = _counters()
    R, color, radii, gb, bb, ib = C_.rasterize_gaussians(rs.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                         rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, H, W, sh_un, 3, rs.campos, False, False,
                                                         options=dict(deterministic_backward=1))
    g = C_.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
                                        rs.kernel_size, rs.subpixel_offset, to_dev(cot), sh_un, 3, rs.campos, gb, R, bb, ib, False,
                                        options=dict(deterministic_backward=1))
    assert _counters() == (f0 + 1, b0 + 1)
    assert torch.equal(color, outs[0]["color"])
    assert torch.equal(C_.view_geometry(gb, P)["bwd_row"], outs[0]["geometry"]["bwd_row"])
    names = ("means2D", "colors_precomp", "opacities", "means3D", "cov3Ds_precomp", "sh", "scales", "rotations")
    # What the row decides is the same bits in both layouts: the rows themselves (above) and dL_dsh.  dL_dmean3D is not compared across
    # layouts: the geometry part of the kernel (not the row's) is compiled once per instantiation under the compiler's default contraction and
    # its fused multiply-adds fall differently in the two, as they did before there was a row; the suite has no switch for the layout.
    differ = [k for k, v in zip(names, g[:8]) if not torch.equal(v, outs[0]["grads_t"][k])]
    print("generic against 16-coefficient layout, tensors that differ:", differ)
    assert torch.equal(g[5], outs[0]["grads_t"]["sh"])
    assert set(differ) <= {"means3D"}, differ      # every other tensor is the same bits in both layouts


# 4 ------------------------------------------------------------------------------------------------------------------------------------
def _lazy_options(_C, **kw):
    for k, v in kw.items():
        _C.set_option(k, v)


@pytest.mark.gpu
def test_rows_of_gaussians_the_lazy_colour_never_coloured():
    """Lazy colour on a split frame: a far Gaussian whose instances no tile asked for is visible and never coloured.  The geometry-only kernel
    leaves it a zero row (and its combined opacity), so nothing is read that was never written: every gradient is finite and, deterministic mode,
    the bits of the frame coloured up front."""
    from diff_gaussian_rasterization import _C
    Wd, Hd = 256, 160
    cam = S.make_camera(Wd, Hd)
    cloud = S.make_cloud(30000, Wd, Hd, sh_degree=3, seed=5, scale_mult=7.0)
    # eight opaque Gaussians in front of the whole frame: every pixel is saturated by near instances, no tile asks for its far ones
    cloud["means3D"][:8] = [(0.0, 0.0, 0.5 + 0.01 * j) for j in range(8)]
    cloud["scales"][:8] = 5.0
    cloud["opacities"][:8] = 0.99
    cot = S.make_cotangent(Wd, Hd)
    saved = {k: _C.get_option(k) for k in ("lazy_sort", "near_split", "near_per_tile", "lazy_min_len", "lazy_target", "lazy_cap", "band_list_min_p",
                                            "lazy_colour", "lazy_colour_min_p")}
    outs = {}
    try:
        for lc in (0, 1):
            _lazy_options(_C, lazy_sort=1, near_split=1, near_per_tile=100, lazy_min_len=256, lazy_target=100, lazy_cap=256, band_list_min_p=1,
                          lazy_colour=lc, lazy_colour_min_p=1)
            f0, b0 = _counters()
            outs[lc] = _native(cloud, cam, 3, cot, deterministic_backward=1)
            assert _counters() == (f0 + 1, b0 + 1)
            sp = outs[lc]["image"]["split"].cpu().numpy().view(np.uint32)
            assert sp[0] != 0xffffffff and sp[1] == 0     # the split is on and no band needed its far instances
    finally:
        for k, v in saved.items():
            _C.set_option(k, v)
    a, b = outs[0], outs[1]
    assert torch.equal(a["color"], b["color"])
    vis = b["radii"] > 0
    never = vis & ~(b["geometry"]["splats"][:, 7:10] != 0).any(dim=1) & ~(a["geometry"]["splats"][:, 7:10] == 0).all(dim=1)
    assert int(never.sum()) > 0             # visible, coloured up front, left uncoloured by the lazy frame
    assert not b["geometry"]["bwd_row"][never][:, :9].any()
    assert torch.equal(b["geometry"]["bwd_row"][:, 9], a["geometry"]["bwd_row"][:, 9])
    for k, v in b["grads_t"].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, a["grads_t"][k]), k


# 5 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cov3d_is_still_written_and_a_precomputed_one_is_read(oracle):
    """The forward kernel writes cov3D through the shared function: the same bits for a plain frame and a raw-parameter frame whether the frame
    leaves rows or not (both instantiations call cov3d_from_scale_rot; that its bits are the previous kernel's holds by construction -- the
    same operations in the same order in a file built without contraction -- and is what the parity suite's cov3D comparisons hold).  With
    cov3D_precomp the backward kernel does not recompute anything: it reads the caller's array, and matches the oracle."""
    cam, cloud, cot = S.make_camera(W, H), _scene(130, 3), S.make_cotangent(W, H)
    a = _native(cloud, cam, 3, cot, forward_only=False)
    b = _native(cloud, cam, 3, None, forward_only=True)
    vis = a["radii"] > 0
    assert torch.equal(a["geometry"]["cov3D"][vis], b["geometry"]["cov3D"][vis])
    # raw-parameter frame: log-scales, unnormalised rotations, logit opacities and a 3-D filter
    rawc = dict(cloud)
    rawc["scales"] = np.log(cloud["scales"]).astype(np.float32)
    rawc["rotations"] = (cloud["rotations"] * 1.7).astype(np.float32)
    rawc["opacities"] = np.log(cloud["opacities"] / (1.0 - cloud["opacities"])).astype(np.float32)
    filt = np.full((130,), 0.01, np.float32)
    ra = _native(rawc, cam, 3, cot, forward_only=False, raw=filt)
    rb = _native(rawc, cam, 3, cot, forward_only=True, raw=filt)
    rvis = ra["radii"] > 0
    assert torch.equal(ra["radii"], rb["radii"]) and torch.equal(ra["geometry"]["cov3D"][rvis], rb["geometry"]["cov3D"][rvis])
    for k in ("scales", "rotations", "opacities", "means3D", "sh"):      # the recomputed covariance against the one read back
        ref = rb["grads"][k]
        assert np.abs(ra["grads"][k] - ref).max() <= GRAD_BOUND * (np.abs(ref).max() + 1e-12), k
    # precomputed covariances: what the forward pass of the plain frame made of scales and rotations
    pre = {k: v for k, v in cloud.items() if k not in ("scales", "rotations")}
    cov = a["geometry"]["cov3D"].cpu().numpy().copy()
    cov[~vis.cpu().numpy()] = np.eye(3, dtype=np.float32)[np.triu_indices(3)] * 1e-4      # (culled rows were never written)
    pre["cov3D_precomp"] = cov
    f0, b0 = _counters()
    hp = _native(pre, cam, 3, cot)
    assert _counters() == (f0 + 1, b0 + 1)
    o = oracle.run_scene(pre, cam, sh_degree=3, cotangent=cot)
    _check_against_oracle(hp["grads"], o, "cov3D_precomp")


# 6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_abi_previous_struct_size_and_the_hint_of_both_bindings():
    """The hint took the four bytes that were padding in front of `options`: wg_forward_args keeps the 288 bytes of its first published layout, and
    a struct as a caller of the previous header fills it (zero-initialised, the field never set) is accepted and leaves rows.  Under
    torch.no_grad() the autograd layer passes the hint through either binding (counted by the library: "backward_row_frames"), and with
    gradients required it does not."""
    from diff_gaussian_rasterization import _C, _abi, GaussianRasterizer
    cam, cloud = S.make_camera(W, H), _scene(65, 3)
    rs = make_settings(cam, 3)
    t = {k: to_dev(v) for k, v in cloud.items()}
    P = 65
    FA = _abi._ForwardArgs
    assert C.sizeof(FA) == 288 and FA.forward_only.offset == FA.binning_capacity.offset + 4 and FA.options.offset == FA.forward_only.offset + 4
    geom, binning, img = _C._Scratch(t["means3D"].device), _C._Scratch(t["means3D"].device), _C._Scratch(t["means3D"].device)
    out_color = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    radii = torch.empty((P,), dtype=torch.int32, device="cuda")
    a = _C._forward_args(geom, binning, img, P, 3, 16, H, W, rs.bg, t["means3D"], t["shs"], None, t["opacities"], t["scales"], 1.0, t["rotations"], None,
                         rs.viewmatrix, rs.projmatrix, rs.campos, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, False, False, out_color, radii,
                         t["means3D"].device)
    assert a.forward_only == 0 and a.struct_size == 288       # the previous header's struct: the same bytes
    f0, _ = _counters()
    rendered = _C._lib.wg_rasterize_forward_ex(C.byref(a))
    gb = geom.take(); binning.take(); img.take()
    assert rendered > 0 and _counters()[0] == f0 + 1
    ref = _native(cloud, cam, 3, None)
    assert torch.equal(out_color, ref["color"])
    assert torch.equal(_C.view_geometry(gb, P)["bwd_row"], ref["geometry"]["bwd_row"])
    a.struct_size = C.sizeof(a) + 8    # a newer caller's struct is refused
    assert _C._lib.wg_rasterize_forward_ex(C.byref(a)) == -1
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    prev = _C.binding_name()
    try:
        for name in ("ctypes", "torch"):
            _C.use_binding(name)       # (an import error of the compiled module fails the test: "both bindings" needs both)
            rast = GaussianRasterizer(rs)
            kw = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                      rotations=t["rotations"])
            f0, _ = _counters()
            c1 = rast(**kw)[0]         # grad mode on, but no input requires a gradient
            f1, _ = _counters()
            kw["shs"] = t["shs"].clone().requires_grad_(True)
            with torch.no_grad():      # an input requires a gradient, but grad mode is off
                c0 = rast(**kw)[0]
            f2, _ = _counters()
            c2 = rast(**kw)[0]
            f3, _ = _counters()
            assert (f1 - f0, f2 - f1, f3 - f2) == (0, 0, 1), name
            assert torch.equal(c0, ref["color"]) and torch.equal(c1, c0) and torch.equal(c2.detach(), c0)
    finally:
        _C.use_binding(prev)


# host only ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 65, 10 ** 6])
def test_geometry_buffer_grows_by_the_row_array(P):
    """The geometry buffer of a frame that leaves rows (wg_geometry_buffer_size_rows) is larger than every other frame's (wg_geometry_buffer_size,
    unchanged) by exactly 40 P bytes rounded up to the carve alignment (256), and the row array is the last thing in it: everything else keeps
    its offset.  The views only do address arithmetic, so a made-up base address serves; wg_view_backward_rows gives no pointer into a buffer
    of the plain size."""
    from diff_gaussian_rasterization import _C
    align = 256
    up = lambda n: (n + align - 1) // align * align
    base = 1 << 30
    v = _C._GeometryView()
    assert _C._lib.wg_view_geometry(C.c_void_p(base), P, C.byref(v)) == 0
    assert v.depths == base
    plain, rows = _C._lib.wg_geometry_buffer_size(P), _C._lib.wg_geometry_buffer_size_rows(P)
    assert rows - plain == up(4 * ROW_FLOATS * P)
    assert v.cov3D - base == up(4 * P) + up(4 * P) + up(48 * P) and v.clamped - v.cov3D == up(24 * P)     # as before the row
    r = C.c_void_p()
    assert _C._lib.wg_view_backward_rows(C.c_void_p(base), P, plain, C.byref(r)) == 0 and not r.value       # a row-less frame's buffer: no rows
    assert _C._lib.wg_view_backward_rows(C.c_void_p(base), P, rows, C.byref(r)) == 0 and r.value
    assert up(r.value - base + 4 * ROW_FLOATS * P) + align == rows                                          # the last array of the buffer
    assert r.value >= base + plain - align and r.value > v.point_offsets                                    # behind all a row-less frame owns
