"""The depth pass (wg_render_depth; csrc/depth/depth.hip: render_depth_kernel): `GaussianRasterizer.forward(..., return_depth=)` returns, as its
last output, one per-Gaussian scalar composited over the finished frame like a colour channel -- one single-channel walk over the frame's
lists instead of a second three-channel rasterizer call.

The judge is bit identity: depth must be `torch.equal` to one channel of the operator's own three-channel call with the scalars as colours over
a zero background.  Only the distance mode (the kernel takes the square root itself) is held to a bound, derived in its test."""
import ctypes as C
import glob
import inspect
import json
import os

import numpy as np
import pytest
import torch

import wg_scenes as S
from wg_testlib import make_settings, rel_err, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
BINDINGS = ["torch", "ctypes"]

# the scenes of tests/test_colour_backward.py: name -> P, W, H, scale_mult, random sub-pixel offsets
SCENES = {
    "ragged": (8000, 250, 130, 3.0, True),        # partial tiles
    "saturating": (1500, 320, 200, 12.0, False),  # long lists, pixels that stop early beside pixels nothing reaches
    "plain": (10000, 256, 256, 1.0, False),
}
BG = (0.2, 0.5, 0.8)
ORDER_BAR = 2e-6   # two orders of the same float32 sums (tests/test_colour_backward.py, docs/OPTIONS.md)


def _scene(name):
    """-> (cloud as device tensors, camera, sub-pixel offsets or None)"""
    if name == "dense":   # ~1000 instances per tile (tests/test_colour_backward.py: _dense)
        P, W, H, sm, offsets, seed = 30000, 320, 200, 7.0, False, 5
    else:
        (P, W, H, sm, offsets), seed = SCENES[name], 11
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=seed, scale_mult=sm).items()}
    so = np.random.default_rng(3).uniform(-0.5, 0.5, size=(H, W, 2)).astype(np.float32) if offsets else None
    return cloud, S.make_camera(W, H), so


def _distances(cloud, cam):
    """the caller's statement (method.py:1621): float32, computed by torch"""
    return torch.norm(cloud["means3D"] - to_dev(cam["campos"])[None], dim=-1)


def _render(cloud, cam, so=None, bg=None, colors=None, **fwd):
    """One call of the operator with precomputed colours -> its output tuple."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=np.zeros(3, np.float32) if bg is None else np.array(bg, np.float32), subpixel_offset=so)
    return GaussianRasterizer(rs)(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"],
                                  colors_precomp=cloud["colors_precomp"] if colors is None else colors, scales=cloud["scales"],
                                  rotations=cloud["rotations"], **fwd)


def _three_channel(cloud, cam, so, values, **fwd):
    """The reference for the bits: the operator's own three-channel call with the scalars as colours over a zero background."""
    img = _render(cloud, cam, so, colors=values[:, None].repeat(1, 3), **fwd)[0]
    assert torch.equal(img[0], img[1]) and torch.equal(img[0], img[2])
    return img[0]


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)


@pytest.fixture()
def options():
    """set_option for the test, the library's defaults back afterwards."""
    from diff_gaussian_rasterization import _C

    def set_(**kw):
        for k, v in kw.items():
            _C.set_option(k, v)
    yield set_
    set_(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, staged_scatter=-1, staged_scatter_cap=0, force_global_sort=0,
         band_list_min_p=2000000, geometry_reuse=_C.GEOMETRY_REUSE_DEFAULT)


# ---- 1. bit identity with the operator's own three-channel call -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("bind", BINDINGS)
def test_depth_has_the_bits_of_a_three_channel_call(binding, bind, exact, name):
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    binding.use_binding(bind)
    cloud, cam, so = _cached(("scene", name), lambda: _scene(name))
    values = _distances(cloud, cam)
    kw = dict(exact_compositing=bool(exact))
    ref = _cached(("three", name, exact), lambda: _three_channel(cloud, cam, so, values, **kw))
    got = _render(cloud, cam, so, return_depth=values, **kw)
    plain = _render(cloud, cam, so, **kw)
    assert len(plain) == 3 and len(got) == 4
    depth = got[-1]
    assert depth.shape == ref.shape and depth.dtype == torch.float32 and not depth.requires_grad
    assert torch.equal(depth, ref)
    assert float(depth.max()) > 0
    for a, b in zip(got[:3], plain):   # color, radii, accumulation: the call without the keyword
        assert torch.equal(a, b)
    # no background term: depth under a background has the bits of depth under none
    assert torch.equal(_render(cloud, cam, so, bg=BG, return_depth=values, **kw)[-1], ref)


# ---- 2. batch edges -------------------------------------------------------------------------------------------------------------------------
def _one_tile(P):
    """One 16 x 16 tile, P faint Gaussians that all cover it: every pixel blends every instance and nothing saturates (alpha ~ 0.009 at
    most: T stays above 0.99^200 = 0.13), so the walk's batches end exactly where the list does."""
    rng = np.random.default_rng(P)
    z = rng.uniform(2.0, 8.0, size=P)
    means = np.stack([0.02 * z * rng.uniform(-1, 1, size=P), 0.02 * z * rng.uniform(-1, 1, size=P), z], axis=1)
    scales = (1.5 * z)[:, None] * np.ones((P, 3))   # ~20 pixels standard deviation on a 16-pixel image
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    cloud = dict(means3D=means, scales=scales, rotations=q, opacities=np.full((P, 1), 0.01), colors_precomp=rng.uniform(0, 1, size=(P, 3)))
    return {k: to_dev(np.ascontiguousarray(v, dtype=np.float32)) for k, v in cloud.items()}, S.make_camera(16, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 200])
def test_batch_edges_on_one_tile(P, exact):
    from wg_testlib import run_hip_native
    cloud, cam = _one_tile(P)
    values = _distances(cloud, cam)
    kw = dict(exact_compositing=bool(exact))
    got = _render(cloud, cam, return_depth=values, **kw)
    assert torch.equal(got[-1], _three_channel(cloud, cam, None, values, **kw))
    if exact:   # the premise: every pixel blended every instance
        n = run_hip_native({k: v.cpu().numpy() for k, v in cloud.items()}, cam, sh_degree=0)["views"]["image"]["n_contrib"]
        assert int(n.min()) == P and int(n.max()) == P
    assert float(got[-1].min()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (17, 33)])
def test_small_and_ragged_images(size):
    W, H = size
    cloud = {k: to_dev(v) for k, v in S.make_cloud(400, W, H, sh_degree=None, seed=2, scale_mult=20.0).items()}
    cam = S.make_camera(W, H)
    values = _distances(cloud, cam)
    depth = _render(cloud, cam, return_depth=values)[-1]
    assert depth.shape == (H, W) and float(depth.max()) > 0
    assert torch.equal(depth, _three_channel(cloud, cam, None, values))


@pytest.mark.gpu
def test_empty_frames_and_pixels_without_a_contributor():
    # every Gaussian behind the camera: all zeros, in both modes
    cloud, cam, so = _cached(("scene", "ragged"), lambda: _scene("ragged"))
    behind = dict(cloud, means3D=cloud["means3D"] * torch.tensor([1.0, 1.0, -1.0], device="cuda"))
    for source in ("distance", _distances(behind, cam)):
        out = _render(behind, cam, so, return_depth=source)
        assert not out[1].any() and out[-1].shape == (130, 250) and not out[-1].any()
    # no Gaussians at all
    z = lambda *s: torch.zeros(*s, device="cuda")
    none = dict(means3D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    for source in ("distance", z(0)):
        out = _render(none, cam, return_depth=source)
        assert len(out) == 4 and out[-1].shape == (130, 250) and not out[-1].any()
    # pixels nothing reaches beside pixels that stopped early: the Gaussians of "saturating" that lie to the right of the image's middle (the
    # whole scene covers every pixel)
    cloud, cam, so = _cached(("scene", "saturating"), lambda: _scene("saturating"))
    keep = cloud["means3D"][:, 0] > 0.15 * cloud["means3D"][:, 2]
    half = {k: v[keep].contiguous() for k, v in cloud.items()}
    values = _distances(half, cam)
    _color, _radii, acc, depth = _render(half, cam, so, return_depth=values)
    untouched, stopped = acc == 0, acc > 1 - 2e-4   # (T within a factor two of the 1e-4 stop)
    assert int(untouched.sum()) > 1000 and int(stopped.sum()) > 1000
    assert not depth[untouched].any() and bool((depth[~untouched] > 0).all())
    assert torch.equal(depth, _three_channel(half, cam, so, values))


# ---- 3. every binning path ------------------------------------------------------------------------------------------------------------------
# tests/test_colour_backward.py: PATHS, and what tests/ref_mode_checks.py: PATHS adds to them
PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256),
         "staged_scatter": dict(staged_scatter=1), "lazy_tiny_fronts": dict(lazy_min_len=256, lazy_target=40, lazy_cap=64),
         "staged_multi_pass": dict(staged_scatter=1, staged_scatter_cap=7), "band_lists": dict(band_list_min_p=1, staged_scatter=0)}


def _default_path(name):
    from wg_testlib import run_hip_native
    cloud, cam, so = _cached(("scene", name), lambda: _scene(name))
    out = dict(distance=_render(cloud, cam, so, return_depth="distance")[-1], values=_render(cloud, cam, so, return_depth=_distances(cloud, cam))[-1])
    rg = run_hip_native({k: v.cpu().numpy() for k, v in cloud.items()}, cam, sh_degree=0, subpixel_offset=so)["views"]["image"]["ranges"].cpu().numpy().astype(np.int64)
    out["longest"] = int((rg[:, 1] - rg[:, 0]).max())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["saturating", "dense"])
def test_every_binning_path_gives_the_same_depth(options, name, path):
    """The walk reads each tile's list up to tile_last only: behind it lie the unsorted tails of lazily sorted lists."""
    base = _cached(("path-default", name), lambda: _default_path(name))   # (the library's defaults: the fixture puts them back after every test)
    cloud, cam, so = _cached(("scene", name), lambda: _scene(name))
    options(**PATHS[path])
    assert torch.equal(_render(cloud, cam, so, return_depth="distance")[-1], base["distance"])
    assert torch.equal(_render(cloud, cam, so, return_depth=_distances(cloud, cam))[-1], base["values"])
    if name == "dense":
        assert base["longest"] > 600


# ---- 4. distance mode against values mode ---------------------------------------------------------------------------------------------------
def _native_frame(_C, rs, cloud, **fwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians(rs.bg, cloud["means3D"], cloud["colors_precomp"], cloud["opacities"], cloud["scales"], cloud["rotations"], 1.0, e,
                                  rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height,
                                  rs.image_width, e, 0, rs.campos, False, False, **fwd)


def _native_depth(_C, rs, cloud, frame, source, **kw):
    return _C.render_depth(frame[3], frame[4], frame[5], frame[0], cloud["means3D"].shape[0], rs.image_height, rs.image_width, source,
                           means3D=cloud["means3D"], campos=rs.campos, subpixel_offset=rs.subpixel_offset, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES) + ["dense"])
def test_distance_mode_against_values_mode(name):
    """`return_depth="distance"` against `return_depth=torch.norm(means3D - campos[None], dim=-1)`, per pixel, within
        (2 n + 7) * 2^-24 * depth_values,      n = the frame's longest walked tile list.
    Derived, not measured (u = 2^-24): each side's distance is within 2.5 u of the true one (three products, two additions, one square root:
    the sum of squares within 0.5 u per product + 0.5 u per addition = at most 1.5 u -- 2.5 u with the rounded differences under the
    squares --, halved by the root, + 0.5 u for the root itself: below 2.5 u), so the two scalars of a Gaussian differ by at most 5 u of
    their value; the blend weights are the same bits on both sides; and a float32 accumulation of at most n positive terms, one fused
    multiply-add each, stays within gamma(n + 1) ~ (n + 1) u of its exact sum, on each side.  5 u + 2 (n + 1) u = (2 n + 7) u."""
    from diff_gaussian_rasterization import _C
    cloud, cam, so = _cached(("scene", name), lambda: _scene(name))
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = _native_frame(_C, rs, cloud)
    n = int(_C.view_image(frame[5], rs.image_height, rs.image_width)["tile_last"].max())
    d_dist = _native_depth(_C, rs, cloud, frame, "distance").double()
    d_val = _native_depth(_C, rs, cloud, frame, _distances(cloud, cam)).double()
    bound = (2 * n + 7) * 2.0 ** -24 * d_val
    diff = (d_dist - d_val).abs()
    covered = d_val > 0
    ratio = float((diff[covered] / bound[covered]).max())
    print(f"{name}: longest walked list {n}, largest |distance - values| / bound = {ratio:.3e}, pixels that differ {int((diff > 0).sum())} of {diff.numel()}")
    if os.environ.get("WG_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "render_depth", "accuracy.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = dict(longest_walked_list=n, bound_factor_ulps=2 * n + 7, largest_ratio_to_bound=ratio,
                          largest_relative_difference=float((diff[covered] / d_val[covered]).max()))
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    assert n > 0 and int(covered.sum()) > 0
    assert bool((diff <= bound).all())
    assert not d_dist[~covered].any()


# ---- 5. no interference ---------------------------------------------------------------------------------------------------------------------
def _step(cloud, cam, so, cot, **fwd):
    """forward + backward through the operator -> (outputs, gradients by name)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=np.array(BG, np.float32), subpixel_offset=so)
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    out = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                 rotations=t["rotations"], **fwd)
    assert out[0].requires_grad and not ("return_depth" in fwd and out[-1].requires_grad)
    out[0].backward(cot)
    return out, dict(means2D=m2d.grad, **{k: v.grad for k, v in t.items()})


@pytest.mark.gpu
def test_the_backward_pass_is_what_it_was(options):
    from diff_gaussian_rasterization import _C
    cloud, cam, so = _cached(("scene", "ragged"), lambda: _scene("ragged"))
    cot = to_dev(S.make_cotangent(250, 130))
    values = _distances(cloud, cam)
    # deterministic mode: the bits
    o0, g0 = _step(cloud, cam, so, cot, deterministic_backward=True)
    o1, g1 = _step(cloud, cam, so, cot, deterministic_backward=True, return_depth=values)
    assert len(o0) == 3 and len(o1) == 4 and torch.equal(o0[0], o1[0])
    for k in g0:
        assert g1[k] is not None and torch.equal(g0[k], g1[k]), k
    # default mode: the image's bits, gradients within two orders of the same atomic sums
    o2, g2 = _step(cloud, cam, so, cot)
    o3, g3 = _step(cloud, cam, so, cot, return_depth=values)
    assert torch.equal(o2[0], o3[0]) and torch.equal(o3[-1], o1[-1])
    for k in g2:
        e = rel_err(g3[k].cpu().numpy(), g2[k].cpu().numpy())
        print(f"default mode, {k}: rel_err with / without return_depth = {e:.3e}")
        assert e <= ORDER_BAR, k
    # grad mode off: a forward_only frame
    with torch.no_grad():
        quiet = _render(cloud, cam, so, bg=BG, return_depth=values)
    assert torch.equal(quiet[-1], o3[-1]) and torch.equal(quiet[0], o3[0].detach())
    # the second of two calls over identical geometry, served by geometry reuse
    from diff_gaussian_rasterization import GaussianRasterizer
    full_distance = _render(cloud, cam, so, return_depth="distance")[-1]
    options(geometry_reuse=1)
    rs = make_settings(cam, 0, subpixel_offset=so)   # (one settings object: the reuse key is the identity of its tensors)
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"])
    hits = _C.geometry_reuse_hits()
    with torch.no_grad():
        GaussianRasterizer(rs)(colors_precomp=torch.rand_like(cloud["colors_precomp"]), **geo)
        reused = GaussianRasterizer(rs)(colors_precomp=cloud["colors_precomp"], return_depth=values, **geo)
        reused_distance = GaussianRasterizer(rs)(colors_precomp=cloud["colors_precomp"], return_depth="distance", **geo)
    assert _C.geometry_reuse_hits() == hits + 2
    options(geometry_reuse=0)
    assert torch.equal(reused[-1], o3[-1]) and torch.equal(reused_distance[-1], full_distance)
    assert torch.equal(reused[0], _render(cloud, cam, so)[0])


@pytest.mark.gpu
def test_every_colour_source_of_the_call():
    """Depth does not depend on the colours: with SH colours, tones, a second colour set and a second tone it is the precomputed-colour call's,
    bit for bit, and the LAST output behind whatever the call returns otherwise; with filter_3D (other geometry: the raw parameters) it is the
    three-channel call's with filter_3D."""
    from diff_gaussian_rasterization import GaussianRasterizer
    P, W, H = 3000, 160, 96
    cam = S.make_camera(W, H)
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=3.0).items()}
    shs = to_dev(S.make_cloud(P, W, H, sh_degree=1, seed=3, scale_mult=3.0)["shs"])
    values = _distances(cloud, cam)
    want = _three_channel(cloud, cam, None, values)
    rs = make_settings(cam, 1)
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"], rotations=cloud["rotations"])
    ones = torch.ones(P, 3, device="cuda")
    sources = dict(shs=(dict(shs=shs), 3), tone=(dict(shs=shs, sh_mul=0.5 * ones, sh_offset=0.1 * ones, sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0), 3),
                   colors_precomp2=(dict(colors_precomp=cloud["colors_precomp"], colors_precomp2=ones), 4),
                   sh_second=(dict(shs=shs, sh_mul=0.5 * ones, sh_second=True, sh_pre_clamp_max2=1.0), 4))
    for name, (kw, arity) in sources.items():
        without = GaussianRasterizer(rs)(**geo, **kw)
        got = GaussianRasterizer(rs)(**geo, **kw, return_depth=values)
        assert len(without) == arity and len(got) == arity + 1, name
        assert torch.equal(got[-1], want), name
        for a, b in zip(got[:-1], without):
            assert torch.equal(a, b), name
    # a second image that takes a gradient while depth does not: the cotangents reach the right places
    c1, c2 = cloud["colors_precomp"].clone().requires_grad_(True), ones.clone().requires_grad_(True)
    img, _r, _a, img2, depth = GaussianRasterizer(rs)(**geo, colors_precomp=c1, colors_precomp2=c2, return_depth="distance")
    (img.sum() + 2 * img2.sum()).backward()
    assert not depth.requires_grad and torch.allclose(c2.grad, 2 * c1.grad, rtol=1e-4, atol=1e-7) and float(c1.grad.abs().max()) > 0
    # raw parameters
    raw = dict(geo, opacities=torch.logit(cloud["opacities"].clamp(0.01, 0.99)), scales=torch.log(cloud["scales"]))
    f3d = torch.full((P, 1), 0.01, device="cuda")
    three = GaussianRasterizer(rs)(**raw, colors_precomp=values[:, None].repeat(1, 3), filter_3D=f3d)[0][0]
    assert torch.equal(GaussianRasterizer(rs)(**raw, colors_precomp=cloud["colors_precomp"], filter_3D=f3d, return_depth=values)[-1], three)


# ---- 6. the native surface, both bindings ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_native_surface_and_refusals_under_both_bindings(binding):
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    cloud, cam, so = _cached(("scene", "ragged"), lambda: _scene("ragged"))
    P, H, W = cloud["means3D"].shape[0], 130, 250
    rs = make_settings(cam, 0, subpixel_offset=so)
    values = _distances(cloud, cam)
    want = _cached(("three", "ragged", 1), lambda: _three_channel(cloud, cam, so, values, exact_compositing=True))
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"], colors_precomp=cloud["colors_precomp"])
    bad = {"wrong size": values[:-1], "float64": values.double(), "host": values.cpu(), "string": "nearest", "number": 3.0}
    said, results = {}, {}
    for name in BINDINGS:
        _C.use_binding(name)
        frame = _native_frame(_C, rs, cloud)
        # into the middle of a larger buffer
        G = 64
        buf = torch.full((G + H * W + G,), float("nan"), device="cuda")
        buf[:G] = 7.0
        buf[-G:] = 9.0
        ret = _native_depth(_C, rs, cloud, frame, values, out=buf[G:G + H * W])
        assert ret.data_ptr() == buf[G:].data_ptr() and ret.shape == (H, W)
        assert bool((buf[:G] == 7.0).all()) and bool((buf[-G:] == 9.0).all()) and not torch.isnan(buf).any()
        assert torch.equal(ret, want)
        again = _native_depth(_C, rs, cloud, frame, values)
        assert torch.equal(again, ret)   # two calls, the same bits
        results[name] = (ret.clone(), _native_depth(_C, rs, cloud, frame, "distance"))
        for case, source in bad.items():
            with pytest.raises(RuntimeError) as info:
                _native_depth(_C, rs, cloud, frame, source)
            said[name, "native", case] = str(info.value)
            with pytest.raises(Exception) as info:
                GaussianRasterizer(rs)(**geo, return_depth=source)
            said[name, "operator", case] = str(info.value)
        with pytest.raises(RuntimeError) as info:   # the frame was composited with exact_compositing = 1
            _native_depth(_C, rs, cloud, frame, values, options=dict(exact_compositing=0))
        said[name, "native", "exact_compositing"] = str(info.value)
        with pytest.raises(Exception) as info:
            GaussianRasterizer(rs)(**geo, return_depth=values, binning_capacity=1_000_000)
        said[name, "operator", "binning_capacity"] = str(info.value)
        # a refused call leaves nothing behind: the well-formed one runs
        assert torch.equal(_native_depth(_C, rs, cloud, frame, values), want)
    for key in [k[1:] for k in said if k[0] == "torch"]:
        assert said[("torch",) + key] == said[("ctypes",) + key], key
    assert said["torch", "native", "wrong size"] == "depth values must have P elements"
    assert {said["torch", "native", c] for c in ("float64", "host", "string", "number")} == {_C.DEPTH_SOURCE_MSG}
    assert {said["torch", "operator", c] for c in ("float64", "host", "string", "number")} == {_C.DEPTH_SOURCE_MSG}
    assert said["torch", "operator", "binning_capacity"] == _C.DEPTH_CAPACITY_MSG
    assert "invalid" in said["torch", "native", "exact_compositing"].lower()
    assert torch.equal(results["torch"][0], results["ctypes"][0]) and torch.equal(results["torch"][1], results["ctypes"][1])


@pytest.mark.gpu
def test_c_abi_struct_size_and_empty_frames():
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _DepthArgs
    cloud, cam, so = _cached(("scene", "ragged"), lambda: _scene("ragged"))
    P, H, W = cloud["means3D"].shape[0], 130, 250
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = _native_frame(_C, rs, cloud)
    values = _distances(cloud, cam).contiguous()
    out = torch.full((H * W + 8,), float("nan"), device="cuda")

    def args(struct_size, P=P, R=frame[0], values=values, buffers=True):
        a = _DepthArgs()
        a.struct_size = struct_size
        a.P, a.R, a.width, a.height = P, R, W, H
        if buffers:
            a.geom_buffer, a.binning_buffer, a.image_buffer = frame[3].data_ptr(), frame[4].data_ptr(), frame[5].data_ptr()
        a.subpixel_offset = rs.subpixel_offset.data_ptr()
        a.values = None if values is None else values.data_ptr()
        a.out_depth, a.stream = out.data_ptr(), torch.cuda.current_stream().cuda_stream
        return a
    full = C.sizeof(_DepthArgs)
    call = lambda a: _C._lib.wg_render_depth(C.byref(a))
    assert call(args(full - 8)) == -1            # a shorter struct than the header's
    assert call(args(full, values=None)) == -1   # neither values nor means3D + campos
    assert call(args(full, R=-1)) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                # a refused call writes nothing
    for kw in (dict(R=0), dict(P=0, R=0, buffers=False, values=None)):
        out.fill_(float("nan"))
        assert call(args(full, **kw)) == 0
        torch.cuda.synchronize()
        assert not out[:H * W].any() and torch.isnan(out[H * W:]).all()
    out.fill_(float("nan"))
    assert call(args(full)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[H * W:]).all()
    assert torch.equal(out[:H * W].view(H, W), _cached(("three", "ragged", 1), lambda: _three_channel(cloud, cam, so, values, exact_compositing=True)))
    assert _C.profile_read().keys() >= {"render_depth"}


# ---- 7. what needs no device ----------------------------------------------------------------------------------------------------------------
def _cpu_call(**fwd):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    P = 5
    rs = GaussianRasterizationSettings(image_height=4, image_width=6, tanfovx=1.0, tanfovy=1.0, kernel_size=0.1, subpixel_offset=torch.zeros(4, 6, 2),
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False, return_accumulation=False)
    return GaussianRasterizer(rs)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), colors_precomp=torch.ones(P, 3),
                                  scales=torch.ones(P, 3), rotations=torch.ones(P, 4), **fwd)


def test_keyword_validation_without_a_device():
    from diff_gaussian_rasterization import _C
    for source in ("nearest", "", 3.0, torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int32), [1.0]):
        with pytest.raises(RuntimeError, match="return_depth must be"):
            _C.check_depth_source(source)
        with pytest.raises(Exception, match="return_depth must be"):   # refused before anything is rendered
            _cpu_call(return_depth=source)
    with pytest.raises(RuntimeError, match="P elements"):
        _C.check_depth_source(torch.zeros(4), 5)
    _C.check_depth_source("distance")
    _C.check_depth_source(torch.zeros(5), 5)
    for source in ("distance", torch.zeros(5)):
        with pytest.raises(Exception) as info:
            _cpu_call(return_depth=source, binning_capacity=100)
        assert str(info.value) == _C.DEPTH_CAPACITY_MSG


def test_output_arity_without_a_device(monkeypatch):
    """`return_depth=None` leaves the outputs of _RasterizeGaussians as they are, and the keyword is the LAST parameter of its forward (after
    every input a backward gradient is returned for) and keyword-only on the public calls.  The native module is replaced by stand-ins:
    only the tuple logic of the autograd function runs."""
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import _C
    fwd = list(inspect.signature(D._RasterizeGaussians.forward).parameters)
    assert fwd[-1] == "return_depth" and inspect.signature(D._RasterizeGaussians.forward).parameters["return_depth"].default is None
    bwd = list(inspect.signature(D._RasterizeGaussians.backward).parameters)
    assert bwd[:5] == ["ctx", "grad_out_color", "_grad_radii", "_grad_accumulation", "grad_out_color2"] and len(bwd) == 6
    for fn in (D.rasterize_gaussians, D.GaussianRasterizer.forward):
        p = inspect.signature(fn).parameters["return_depth"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    calls = []

    def fake_forward(*a, colors2=None, **kw):
        e = torch.empty(0, dtype=torch.uint8)
        return (7, torch.zeros(3, 4, 6), torch.zeros(5, dtype=torch.int32), e, e, e) + ((torch.ones(3, 4, 6),) if colors2 is not None else ())

    def fake_depth(geom, binning, img, R, P, H, W, source, *a, **kw):
        calls.append((R, P, H, W, source if isinstance(source, str) else tuple(source.shape)))
        return torch.full((H, W), 2.0)
    monkeypatch.setattr(_C, "rasterize_gaussians", fake_forward)
    monkeypatch.setattr(_C, "render_depth", fake_depth)
    assert len(_cpu_call()) == 3 and len(_cpu_call(return_depth=None)) == 3 and not calls
    assert len(_cpu_call(colors_precomp2=torch.ones(5, 3))) == 4 and not calls
    out = _cpu_call(return_depth="distance")
    assert len(out) == 4 and out[-1].shape == (4, 6) and float(out[-1][0, 0]) == 2.0 and not out[-1].requires_grad
    out = _cpu_call(return_depth=torch.zeros(5), colors_precomp2=torch.ones(5, 3))
    assert len(out) == 5 and float(out[3][0, 0, 0]) == 1.0 and float(out[-1][0, 0]) == 2.0
    assert calls == [(7, 5, 4, 6, "distance"), (7, 5, 4, 6, (5,))]
