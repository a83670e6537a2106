"""The contribution pass (wg_render_contributions; csrc/contrib/contrib.hip: render_contrib_kernel): `GaussianRasterizer.forward(...,
contributions=stats)` combines into caller-owned [P] arrays, for every Gaussian and over the (pixel, Gaussian) pairs the frame blended, the
largest blend weight w = alpha * T, the number of pairs and the sum of floor(w * 2^32).

The yardstick is the operator's own forward call with one-hot precomputed colours over a zero background (tests/contributions_lib.py):
channel c of that image IS Gaussian g_c's blend weight per pixel, bit for bit.  Every comparison with it is `torch.equal`; there is no
tolerance anywhere but in the one float64 cross-check of the summed weight, whose bound is derived in its test."""
import ctypes as C
import glob
import inspect
import json
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch

import wg_scenes as S
import contributions_lib as L
from wg_testlib import make_settings, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
BINDINGS = ["torch", "ctypes"]
BG = (0.2, 0.5, 0.8)

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _scene(name):
    return _cached(("scene", name), lambda: L.scene(name))


@pytest.fixture(scope="module", autouse=True)
def _release_what_the_module_cached():
    """The scenes, frames and statistics the tests share live as long as this module's tests run, not as long as the process."""
    yield
    _cache.clear()


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)


@pytest.fixture()
def options():
    """set_option for the test, the library's defaults back afterwards (tests/test_render_depth.py's fixture, restated)."""
    from diff_gaussian_rasterization import _C
    order_before = _C.get_option("forward_order")

    def set_(**kw):
        for k, v in kw.items():
            _C.set_option(k, v)
    yield set_
    set_(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, staged_scatter=-1, staged_scatter_cap=0, force_global_sort=0,
         band_list_min_p=2000000, geometry_reuse=_C.GEOMETRY_REUSE_DEFAULT, forward_order=order_before)


def _triple(stats):
    return stats.max_weight, stats.hits, stats.weight_sum_q32


def _same(a, b):
    """two ContributionStats (or triples) hold the same bits"""
    a, b = (_triple(x) if not isinstance(x, tuple) else x for x in (a, b))
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- 1. one-tile scenes: batch edges --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 200])
def test_one_tile_scenes_equal_the_one_hot_yardstick(P, exact):
    cloud, cam = L.one_tile(P)
    kw = dict(exact_compositing=bool(exact))
    stats, _out = L.collect(cloud, cam, **kw)
    want = L.yardstick(cloud, cam, None, list(range(P)), **kw)
    L.assert_stats_equal(stats, want)
    assert stats.views == 1
    assert bool((stats.hits == 256).all())   # the recipe's premise: every pixel blended every instance
    assert float(stats.max_weight.min()) > 0 and int(stats.weight_sum_q32.min()) > 0


# ---- 2. multi-tile scenes -------------------------------------------------------------------------------------------------------------------
def _scene_stats(name, exact):
    cloud, cam, so = _scene(name)
    stats, out = L.collect(cloud, cam, so, exact_compositing=bool(exact))
    return stats, out


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("name", list(L.SCENES))
def test_multi_tile_scenes_equal_the_one_hot_yardstick(name, exact):
    cloud, cam, so = _scene(name)
    P, W, H = cloud["means3D"].shape[0], cam["width"], cam["height"]
    stats, out = _cached(("stats", name, exact), lambda: _scene_stats(name, exact))
    radii = out[1]
    visible = torch.nonzero(radii > 0).flatten().cpu().numpy()
    ids = sorted(int(i) for i in np.random.default_rng(7).choice(visible, size=96, replace=False))   # 32 one-hot calls
    want = L.yardstick(cloud, cam, so, ids, exact_compositing=bool(exact))
    L.assert_stats_equal(stats, want, ids)
    assert int((want[1] > 0).sum()) >= 24   # the subset is not vacuous: a good part of it was blended somewhere
    # over all P
    mw, hits, q = _triple(stats)
    assert torch.equal(hits > 0, mw > 0) and torch.equal(hits > 0, q > 0)
    assert bool((radii[hits > 0] > 0).all())
    assert float(mw.max()) <= 0.99
    assert bool((q <= hits * (1 << 32)).all()) and bool((hits <= H * W).all()) and bool((hits >= 0).all())
    assert int((hits > 0).sum()) > P // 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(L.SCENES))
def test_summed_weight_against_an_all_ones_render(name):
    """In float64, sum_g weight_sum equals the pixel sum of a render with every colour 1 (each channel: sum of w per pixel) within
        pixels * n * 2^-24  +  hits * 2^-32,       n = the frame's longest walked tile list.
    Derived, not measured: the render adds at most n weights per pixel with one fused multiply-add each; every partial sum is at most 1 (it is
    1 - T), so each rounding is at most 2^-25 and a pixel is within n * 2^-24 of its exact sum with a factor two to spare; the fixed-point
    side truncates each term by less than 2^-32 and adds exactly."""
    from diff_gaussian_rasterization import _C
    cloud, cam, so = _scene(name)
    W, H = cam["width"], cam["height"]
    stats, _out = _cached(("stats", name, 1), lambda: _scene_stats(name, 1))
    ones = L.render(cloud, cam, so, colors=torch.ones_like(cloud["colors_precomp"]))[0][0]
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = L.native_frame(_C, rs, cloud)
    n = int(_C.view_image(frame[5], H, W)["tile_last"].max())
    total_hits = int(stats.hits.sum())
    bound = H * W * n * 2.0 ** -24 + total_hits * 2.0 ** -32
    got, want = float(stats.weight_sum.sum()), float(ones.double().sum())
    ratio = abs(got - want) / bound
    print(f"{name}: sum of weight_sum {got:.9f}, all-ones render {want:.9f}, |difference| / bound = {ratio:.3e} (n = {n}, hits = {total_hits})")
    if os.environ.get("WG_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "contributions", "accuracy.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = dict(longest_walked_list=n, hits=total_hits, pixels=H * W, sum_of_weight_sum=got, all_ones_render_sum=want, bound=bound,
                          ratio_to_bound=ratio)
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    assert n > 0 and want > 0
    assert abs(got - want) <= bound


# ---- 3. the mask ----------------------------------------------------------------------------------------------------------------------------
def _masks(H, W):
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    return dict(half=(xx < W // 2).float(), checker=(((xx + yy) % 2) == 0).float())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["half", "checker"])
@pytest.mark.parametrize("case", ["tile65", "17x33"])
def test_masked_pixels_take_no_part(case, kind):
    if case == "tile65":
        cloud, cam = L.one_tile(65)
    else:
        W, H = 17, 33
        cloud = {k: to_dev(v) for k, v in S.make_cloud(400, W, H, sh_degree=None, seed=2, scale_mult=20.0).items()}
        cam = S.make_camera(W, H)
    P, W, H = cloud["means3D"].shape[0], cam["width"], cam["height"]
    mask = _masks(H, W)[kind]
    stats, _ = L.collect(cloud, cam, mask=mask)
    ids = list(range(P)) if P <= 65 else sorted(int(i) for i in np.random.default_rng(1).choice(P, size=48, replace=False))
    want = L.yardstick(cloud, cam, None, ids, mask=mask)
    L.assert_stats_equal(stats, want, ids)
    assert int(stats.hits.sum()) > 0
    assert bool((stats.hits <= int(mask.sum())).all())
    # a bool mask and a [1, H, W] one are accepted and converted
    for other in (mask.bool(), mask[None], mask.bool()[None]):
        assert _same(L.collect(cloud, cam, mask=other)[0], stats)
    # an all-zero mask leaves everything zero; -0.0f masks like 0.0f
    for zero in (torch.zeros(H, W, device="cuda"), -torch.zeros(H, W, device="cuda")):
        none, _ = L.collect(cloud, cam, mask=zero)
        assert not none.max_weight.any() and not none.hits.any() and not none.weight_sum_q32.any() and none.views == 1
    signed = torch.where(mask != 0, mask, -torch.zeros_like(mask))
    assert bool(torch.signbit(signed).any())
    assert _same(L.collect(cloud, cam, mask=signed)[0], stats)
    # and an all-ones mask is no mask
    assert _same(L.collect(cloud, cam, mask=torch.ones(H, W, device="cuda"))[0], L.collect(cloud, cam)[0])


# ---- 4. accumulation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accumulation_over_views_and_overwriting():
    from diff_gaussian_rasterization import ContributionStats, _C
    cloud, cam, so = _scene("ragged")
    P, W, H = cloud["means3D"].shape[0], cam["width"], cam["height"]
    cam2 = S.make_camera(W, H, yaw_deg=9.0)
    a, _ = L.collect(cloud, cam, so)
    b, _ = L.collect(cloud, cam2, so)
    assert not _same(a, b)
    both = ContributionStats(P, "cuda")
    L.collect(cloud, cam, so, stats=both)
    L.collect(cloud, cam2, so, stats=both)
    assert both.views == 2
    assert _same(both, (torch.maximum(a.max_weight, b.max_weight), a.hits + b.hits, a.weight_sum_q32 + b.weight_sum_q32))
    merged = ContributionStats(P, "cuda").merge_(a).merge_(b)
    assert _same(merged, both) and merged.views == 2
    twice = ContributionStats(P, "cuda")
    L.collect(cloud, cam, so, stats=twice)
    L.collect(cloud, cam, so, stats=twice)
    assert twice.views == 2 and _same(twice, (a.max_weight, 2 * a.hits, 2 * a.weight_sum_q32))
    # accumulate = 0 overwrites poisoned arrays; accumulate = 1 combines into them
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = L.native_frame(_C, rs, cloud)
    out = L.fresh(P, poison=True)
    L.native_contrib(_C, rs, P, frame, *out, accumulate=False)
    assert _same(out, a)
    out = L.fresh(P, poison=True)
    L.native_contrib(_C, rs, P, frame, *out, accumulate=True)
    assert _same(out, (torch.clamp(a.max_weight, min=0.5), a.hits + 77, a.weight_sum_q32 + (1 << 40)))


# ---- 5. the frame is untouched --------------------------------------------------------------------------------------------------------------
def _step(cloud, cam, so, cot, **fwd):
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=np.array(BG, np.float32), subpixel_offset=so)
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    out = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                 rotations=t["rotations"], **fwd)
    out[0].backward(cot)
    return out, dict(means2D=m2d.grad, **{k: v.grad for k, v in t.items()})


@pytest.mark.gpu
def test_the_frame_and_its_backward_pass_are_what_they_were(options):
    from diff_gaussian_rasterization import ContributionStats, GaussianRasterizer, _C
    cloud, cam, so = _scene("ragged")
    P = cloud["means3D"].shape[0]
    cot = to_dev(S.make_cotangent(250, 130))
    alone, _ = L.collect(cloud, cam, so)
    plain = L.render(cloud, cam, so, bg=BG)
    stats, with_kw = L.collect(cloud, cam, so, bg=BG)
    assert len(plain) == 3 and len(with_kw) == 3
    for x, y in zip(plain, with_kw):
        assert torch.equal(x, y)
    assert _same(stats, alone)   # (no background term in a blend weight)
    # a step's gradients, bit for bit, in the deterministic mode
    o0, g0 = _step(cloud, cam, so, cot, deterministic_backward=True)
    s1 = ContributionStats(P, "cuda")
    o1, g1 = _step(cloud, cam, so, cot, deterministic_backward=True, contributions=s1)
    assert len(o1) == 3 and torch.equal(o0[0], o1[0]) and o1[0].requires_grad
    for k in g0:
        assert g1[k] is not None and torch.equal(g0[k], g1[k]), k
    assert _same(s1, alone)
    # return_depth beside it is unchanged, and stays the last output
    depth = L.render(cloud, cam, so, return_depth="distance")[-1]
    s2 = ContributionStats(P, "cuda")
    got = L.render(cloud, cam, so, return_depth="distance", contributions=s2)
    assert len(got) == 4 and torch.equal(got[-1], depth) and _same(s2, alone)
    # grad mode off (a forward_only frame)
    with torch.no_grad():
        quiet, _ = L.collect(cloud, cam, so)
    assert _same(quiet, alone)
    # every colour source: SH colours, a second colour set; and the second of two calls served by geometry reuse
    rs = make_settings(cam, 1, subpixel_offset=so)
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"])
    shs = to_dev(S.make_cloud(P, 250, 130, sh_degree=1, seed=11, scale_mult=3.0)["shs"])
    ones = torch.ones(P, 3, device="cuda")
    for kw, arity in ((dict(shs=shs), 3), (dict(colors_precomp=cloud["colors_precomp"], colors_precomp2=ones), 4),
                      (dict(shs=shs, sh_mul=0.5 * ones, sh_second=True, sh_pre_clamp_max2=1.0), 4)):
        s = ContributionStats(P, "cuda")
        out = GaussianRasterizer(rs)(**geo, **kw, contributions=s)
        assert len(out) == arity and _same(s, alone), list(kw)
    options(geometry_reuse=1)
    hits = _C.geometry_reuse_hits()
    s3 = ContributionStats(P, "cuda")
    with torch.no_grad():
        GaussianRasterizer(rs)(colors_precomp=torch.rand_like(cloud["colors_precomp"]), **geo)
        GaussianRasterizer(rs)(colors_precomp=cloud["colors_precomp"], contributions=s3, **geo)
    assert _C.geometry_reuse_hits() == hits + 1
    options(geometry_reuse=0)
    assert _same(s3, alone)


# ---- 6. reproducibility and paths -----------------------------------------------------------------------------------------------------------
PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256),
         "staged_scatter": dict(staged_scatter=1), "lazy_tiny_fronts": dict(lazy_min_len=256, lazy_target=40, lazy_cap=64),
         "staged_multi_pass": dict(staged_scatter=1, staged_scatter_cap=7), "band_lists": dict(band_list_min_p=1, staged_scatter=0)}


def _default_path(name):
    cloud, cam, so = _scene(name)
    return L.collect(cloud, cam, so)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["saturating", "dense"])
def test_every_binning_path_gives_the_same_bits(options, name, path):
    base = _cached(("path-default", name), lambda: _default_path(name))   # (the library's defaults: the fixture puts them back after every test)
    cloud, cam, so = _scene(name)
    options(**PATHS[path])
    assert _same(L.collect(cloud, cam, so)[0], base)
    assert int(base.hits.sum()) > 0


@pytest.mark.gpu
def test_two_calls_and_another_launch_order_give_the_same_bits(options):
    cloud, cam, so = _scene("saturating")
    options(forward_order=0)
    first = L.collect(cloud, cam, so)[0]
    assert _same(L.collect(cloud, cam, so)[0], first)
    options(forward_order=1)   # from the second frame on the forward kernel launches its tiles in the order the camera's history suggests
    for _ in range(3):
        assert _same(L.collect(cloud, cam, so)[0], first)


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_frames_tiny_images_and_a_nan_opacity():
    from diff_gaussian_rasterization import ContributionStats
    cloud, cam, so = _scene("ragged")
    # a frame with R = 0: every Gaussian behind the camera
    behind = dict(cloud, means3D=cloud["means3D"] * torch.tensor([1.0, 1.0, -1.0], device="cuda"))
    stats, out = L.collect(behind, cam, so)
    assert not out[1].any() and stats.views == 1 and not stats.hits.any() and not stats.max_weight.any() and not stats.weight_sum_q32.any()
    # P = 0
    z = lambda *s: torch.zeros(*s, device="cuda")
    none = dict(means3D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    stats, out = L.collect(none, cam)
    assert len(out) == 3 and stats.views == 1 and stats.hits.numel() == 0
    # a 1 x 1 image
    tiny = {k: to_dev(v) for k, v in S.make_cloud(400, 1, 1, sh_degree=None, seed=2, scale_mult=20.0).items()}
    cam1 = S.make_camera(1, 1)
    stats, _ = L.collect(tiny, cam1)
    ids = [int(i) for i in torch.nonzero(stats.hits).flatten()[:9]] + [0, 1, 2]
    L.assert_stats_equal(stats, L.yardstick(tiny, cam1, None, ids), ids)
    assert int(stats.hits.max()) == 1 and int(stats.hits.sum()) > 0
    # one NaN opacity: the reference blends such a Gaussian (alpha = min(0.99f, NaN) = 0.99f) wherever its tile rectangle reaches; whatever
    # weight the forward call gave it -- finite or NaN -- the pass reports by the rules of contributions_lib.stats_of_weights
    cloudn, camn = L.one_tile(65)
    cloudn = dict(cloudn, opacities=cloudn["opacities"].clone())
    cloudn["opacities"][30] = float("nan")
    stats, _ = L.collect(cloudn, camn)
    L.assert_stats_equal(stats, L.yardstick(cloudn, camn, None, list(range(65))))
    assert int(stats.hits[30]) > 0
    mw = float(stats.max_weight[30])
    assert mw != mw or mw > 0.5   # NaN, or the 0.99 blend


@pytest.mark.gpu
def test_guard_words_and_null_outputs_through_the_native_call(binding):
    _C = binding
    cloud, cam, so = _scene("ragged")
    P = cloud["means3D"].shape[0]
    rs = make_settings(cam, 0, subpixel_offset=so)
    want = _triple(L.collect(cloud, cam, so)[0])
    for name in BINDINGS:
        _C.use_binding(name)
        frame = L.native_frame(_C, rs, cloud)
        G = 16
        bufs = [torch.full((G + P + G,), 3.0, device="cuda"), torch.full((G + P + G,), 5, dtype=torch.int64, device="cuda"),
                torch.full((G + P + G,), 7, dtype=torch.int64, device="cuda")]
        L.native_contrib(_C, rs, P, frame, *(b[G:G + P] for b in bufs), accumulate=False)
        for b, w, guard in zip(bufs, want, (3.0, 5, 7)):
            assert bool((b[:G] == guard).all()) and bool((b[-G:] == guard).all())
            assert torch.equal(b[G:G + P], w)
        # each output pointer NULL in turn: the other two are what they were
        for skip in range(3):
            out = list(L.fresh(P, poison=True))
            out[skip] = None
            L.native_contrib(_C, rs, P, frame, *out, accumulate=False)
            for k in range(3):
                assert out[k] is None or torch.equal(out[k], want[k]), (name, skip, k)


# ---- 8. the surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_native_surface_and_refusals_under_both_bindings(binding):
    _C = binding
    from diff_gaussian_rasterization import ContributionStats, GaussianRasterizer
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    cloud, cam, so = _scene("ragged")
    P, H, W = cloud["means3D"].shape[0], 130, 250
    rs = make_settings(cam, 0, subpixel_offset=so)
    geo = dict(means3D=cloud["means3D"], means2D=torch.zeros_like(cloud["means3D"]), opacities=cloud["opacities"], scales=cloud["scales"],
               rotations=cloud["rotations"], colors_precomp=cloud["colors_precomp"])
    mask = _masks(H, W)["checker"]
    said, results = {}, {}
    for name in BINDINGS:
        _C.use_binding(name)
        frame = L.native_frame(_C, rs, cloud)
        calls = _C.get_option("contribution_calls")
        out, outm = L.fresh(P), L.fresh(P)
        assert L.native_contrib(_C, rs, P, frame, *out) is None
        L.native_contrib(_C, rs, P, frame, *outm, mask=mask)
        assert _C.get_option("contribution_calls") == calls + 2
        results[name] = (out, outm)
        bad = {"all None": (None, None, None), "float64 max": (out[0].double(), out[1], out[2]), "int32 hits": (out[0], out[1].int(), out[2]),
               "short sum": (out[0], out[1], out[2][:-1]), "host hits": (out[0], out[1].cpu(), out[2]), "strided max": (torch.zeros(2 * P, device="cuda")[::2], out[1], out[2])}
        for case, triple in bad.items():
            with pytest.raises(RuntimeError) as info:
                L.native_contrib(_C, rs, P, frame, *triple)
            said[name, case] = str(info.value)
        for case, m in {"mask size": mask[:-1], "mask dtype": mask.double(), "mask host": mask.cpu()}.items():
            with pytest.raises(RuntimeError) as info:
                L.native_contrib(_C, rs, P, frame, *out, mask=m)
            said[name, case] = str(info.value)
        with pytest.raises(RuntimeError) as info:   # the frame was composited with exact_compositing = 1
            L.native_contrib(_C, rs, P, frame, *out, options=dict(exact_compositing=0))
        said[name, "exact_compositing"] = str(info.value)
        with pytest.raises(Exception) as info:
            GaussianRasterizer(rs)(**geo, contributions=ContributionStats(P, "cuda"), binning_capacity=1_000_000)
        said[name, "binning_capacity"] = str(info.value)
        # a refused call leaves nothing behind: the well-formed one runs and gives the first one's bits
        again = L.fresh(P)
        L.native_contrib(_C, rs, P, frame, *again)
        assert _same(again, results[name][0])
    for key in [k[1] for k in said if k[0] == "torch"]:
        assert said["torch", key] == said["ctypes", key], key
    assert said["torch", "all None"] == _C.CONTRIB_NONE_MSG
    assert said["torch", "float64 max"] == said["torch", "strided max"] == "max_weight must be a contiguous float32 tensor of P elements on the frame's HIP device"
    assert said["torch", "int32 hits"] == said["torch", "host hits"] == "hits must be a contiguous int64 tensor of P elements on the frame's HIP device"
    assert said["torch", "short sum"] == "weight_sum_q32 must be a contiguous int64 tensor of P elements on the frame's HIP device"
    assert {said["torch", c] for c in ("mask size", "mask dtype", "mask host")} == {_C.CONTRIB_MASK_MSG}
    assert said["torch", "binning_capacity"] == _C.CONTRIB_CAPACITY_MSG
    assert "invalid" in said["torch", "exact_compositing"].lower()
    assert _same(results["torch"][0], results["ctypes"][0]) and _same(results["torch"][1], results["ctypes"][1])
    assert int(results["torch"][0][1].sum()) > int(results["torch"][1][1].sum()) > 0


@pytest.mark.gpu
def test_c_abi_struct_size_refusals_stage_and_counter():
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _CallOptions, _ContribArgs
    cloud, cam, so = _scene("ragged")
    P, H, W = cloud["means3D"].shape[0], 130, 250
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = L.native_frame(_C, rs, cloud)
    want = _triple(L.collect(cloud, cam, so)[0])
    out = L.fresh(P, poison=True)
    poison = [t.clone() for t in out]
    fast = _CallOptions(0, 0, 1)

    def args(struct_size, P=P, R=frame[0], outs=(0, 1, 2), buffers=True, accumulate=0, options=None):
        a = _ContribArgs()
        a.struct_size = struct_size
        a.P, a.R, a.width, a.height = P, R, W, H
        if buffers:
            a.geom_buffer, a.binning_buffer, a.image_buffer = frame[3].data_ptr(), frame[4].data_ptr(), frame[5].data_ptr()
        a.subpixel_offset = rs.subpixel_offset.data_ptr()
        for k, n in enumerate(("max_weight", "hits", "weight_sum_q32")):
            setattr(a, n, out[k].data_ptr() if k in outs else None)
        a.accumulate, a.stream = accumulate, torch.cuda.current_stream().cuda_stream
        if options is not None:
            a.options = C.pointer(options)
        return a
    full = C.sizeof(_ContribArgs)
    call = lambda a: _C._lib.wg_render_contributions(C.byref(a))
    calls = _C.get_option("contribution_calls")
    assert call(args(full - 8)) == -1                # a shorter struct than the header's
    assert call(args(full, outs=())) == -1           # all three outputs NULL
    assert call(args(full, R=-1)) == -1
    assert call(args(full, accumulate=2)) == -1
    assert call(args(full, buffers=False)) == -1
    assert call(args(full, options=fast)) == -1      # the frame was composited with exact_compositing = 1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, poison))   # a refused call writes nothing
    assert _C.get_option("contribution_calls") == calls
    assert call(args(full, R=0)) == 0                # no lists to walk: WG_OK after the zero fill
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in out) and _C.get_option("contribution_calls") == calls
    assert call(args(full, P=0, R=0, buffers=False)) == 0
    _C.profile_enable(True)
    try:
        _C.profile_reset()
        assert call(args(full)) == 0
        torch.cuda.synchronize()
        prof = _C.profile_read()
    finally:
        _C.profile_enable(False)
    assert _same(tuple(out), want)
    assert _C.get_option("contribution_calls") == calls + 1
    assert prof["render_contributions"][1] == 1 and prof["render_contributions"][0] > 0


@pytest.mark.gpu
def test_a_captured_replay_on_one_stream_gives_the_eager_bits():
    from diff_gaussian_rasterization import _C
    cloud, cam, so = _scene("saturating")
    P = cloud["means3D"].shape[0]
    rs = make_settings(cam, 0, subpixel_offset=so)
    frame = L.native_frame(_C, rs, cloud)
    want = L.fresh(P)
    L.native_contrib(_C, rs, P, frame, *want)
    out = L.fresh(P, poison=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up on the capture stream
            L.native_contrib(_C, rs, P, frame, *out, accumulate=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.native_contrib(_C, rs, P, frame, *out, accumulate=False)
    for t in out:
        t.fill_(9)
    for _ in range(2):   # each replay zero-fills first: the second gives the first's bits, not their double
        graph.replay()
    torch.cuda.synchronize()
    assert _same(out, want) and int(want[1].sum()) > 0


# ---- 9. what it is for ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pruning_what_was_never_blended_changes_no_pixel():
    """Sweep three cameras, drop every Gaussian with hits == 0, render again: the blended pairs of every pixel are the same ones in the same
    order (pruning keeps the relative order of the rows; the per-tile sort is by depth, then row), so colour and accumulation are the same
    bits.  (A Gaussian that was never blended can still be the instance a pixel STOPS at -- it is then not blended there -- and without it
    such a pixel would go on to the next instance; the cloud is the sparse one, scale_mult 1, in which no pixel of these views saturates:
    asserted below through the accumulation, T >= 1e-4 / (1 - 0.99) = 1e-2 being necessary for no stop to have been taken.)"""
    from diff_gaussian_rasterization import ContributionStats
    P, W, H = 10000, 256, 256
    cloud = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=11, scale_mult=1.0).items()}
    cams = [S.make_camera(W, H, yaw_deg=y) for y in (0.0, 15.0, 35.0)]
    stats = ContributionStats(P, "cuda")
    before = []
    with torch.no_grad():
        for cam in cams:
            before.append(L.collect(cloud, cam, stats=stats)[1])
    assert stats.views == 3
    keep = stats.keep_mask(min_hits=1)
    removed = int((~keep).sum())
    assert 0 < removed < P
    assert all(float(o[2].max()) < 1.0 - 1e-2 for o in before)   # the docstring's premise: no pixel got near the stop
    pruned = {k: v[keep].contiguous() for k, v in cloud.items()}
    with torch.no_grad():
        for cam, o in zip(cams, before):
            color, radii, acc = L.render(pruned, cam)
            assert torch.equal(color, o[0]) and torch.equal(acc, o[2])
            assert torch.equal(radii, o[1][keep])
    # and the pruned cloud's own statistics are the kept rows'
    again = ContributionStats(int(keep.sum()), "cuda")
    with torch.no_grad():
        for cam in cams:
            L.collect(pruned, cam, stats=again)
    assert _same(again, (stats.max_weight[keep], stats.hits[keep], stats.weight_sum_q32[keep]))
    assert bool((again.hits > 0).all())


# ---- 10. the caller -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_prune_by_contribution_on_the_real_caller():
    import math
    caller_dir = os.path.join(ROOT, "tests", "real_caller")
    added = caller_dir not in sys.path
    if added:
        sys.path.insert(0, caller_dir)
    try:
        import harness
    finally:
        if added:
            sys.path.remove(caller_dir)
    import wg_integration
    from diff_gaussian_rasterization import _C
    # (no seeding: the process-wide generators are left as they were; whichever cameras the three steps draw, the assertions below hold)
    _m, wg = harness.make_caller(20_000, 320, 240, n_cams=3)
    for step in range(3):
        assert math.isfinite(wg.train_iteration(step)["loss"])
    model = wg.model
    P = model.xyz.shape[0]
    calls = _C.get_option("contribution_calls")
    r = wg_integration.prune_by_contribution(wg, wg.train_cameras, min_hits=1)
    assert _C.get_option("contribution_calls") == calls + 3   # one pass per camera: the FIRST rasterizer call of each render only
    assert 0 < r < P
    for group in model.optimizer.param_groups:
        p = group["params"][0]
        if p.shape[0] in (P, P - r):   # a per-Gaussian parameter
            assert p.shape[0] == P - r, group.get("name")
            st = model.optimizer.state.get(p)
            if st:
                assert st["exp_avg"].shape[0] == P - r and st["exp_avg_sq"].shape[0] == P - r, group.get("name")
    assert model.xyz.shape[0] == P - r
    for n in ("xyz_grad", "denom", "max_radii2D", "filter_3D"):
        if hasattr(model, n):
            assert getattr(model, n).shape[0] == P - r, n
    assert math.isfinite(wg.train_iteration(3)["loss"])
    with pytest.raises(ValueError):
        wg_integration.prune_by_contribution(wg, wg.train_cameras)


# ---- what needs no device -------------------------------------------------------------------------------------------------------------------
def _cpu_call(**fwd):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    P = 5
    rs = GaussianRasterizationSettings(image_height=4, image_width=6, tanfovx=1.0, tanfovy=1.0, kernel_size=0.1, subpixel_offset=torch.zeros(4, 6, 2),
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False, return_accumulation=False)
    return GaussianRasterizer(rs)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), colors_precomp=torch.ones(P, 3),
                                  scales=torch.ones(P, 3), rotations=torch.ones(P, 4), **fwd)


@pytest.fixture()
def fake_native(monkeypatch):
    """The native calls replaced by stand-ins (as tests/test_render_depth.py: test_output_arity_without_a_device): only the Python logic runs."""
    from diff_gaussian_rasterization import _C
    log = dict(forward=0, contrib=[])

    def fake_forward(*a, colors2=None, **kw):
        log["forward"] += 1
        e = torch.empty(0, dtype=torch.uint8)
        return (7, torch.zeros(3, 4, 6), torch.zeros(5, dtype=torch.int32), e, e, e) + ((torch.ones(3, 4, 6),) if colors2 is not None else ())

    def fake_contrib(geom, binning, img, R, P, H, W, max_weight, hits, q32, mask, so, options=None, accumulate=True, debug=False):
        log["contrib"].append(dict(R=R, P=P, H=H, W=W, mask=None if mask is None else mask.clone(), accumulate=accumulate))
        hits += 1
    monkeypatch.setattr(_C, "rasterize_gaussians", fake_forward)
    monkeypatch.setattr(_C, "render_contributions", fake_contrib)
    monkeypatch.setattr(_C, "render_depth", lambda geom, binning, img, R, P, H, W, source, *a, **kw: torch.full((H, W), 2.0))
    return log


def test_keywords_are_keyword_only_and_validated_before_anything_is_rendered(fake_native):
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import ContributionStats, _C, contributions as CM
    for fn in (D.rasterize_gaussians, D.GaussianRasterizer.forward):
        for n in ("contributions", "contribution_mask"):
            p = inspect.signature(fn).parameters[n]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(D._RasterizeGaussians.forward).parameters)[-1] == "return_depth"   # (still the last one)
    good = ContributionStats(5, "cpu")
    wrong_dtype, wrong_layout = ContributionStats(5, "cpu"), ContributionStats(5, "cpu")
    wrong_dtype.hits = wrong_dtype.hits.int()
    wrong_layout.max_weight = torch.zeros(10)[::2]
    for bad in (torch.zeros(5), "stats", 3, ContributionStats(4, "cpu"), wrong_dtype, wrong_layout, ContributionStats(5, "meta")):
        with pytest.raises(Exception) as info:
            _cpu_call(contributions=bad)
        assert str(info.value) == CM.STATS_MSG
    for bad in (torch.zeros(4, 5), torch.zeros(4, 6, dtype=torch.float64), torch.zeros(2, 4, 6), torch.zeros(4, 6, dtype=torch.int32), [[1.0]],
                torch.zeros(4, 6, device="meta")):
        with pytest.raises(Exception) as info:
            _cpu_call(contributions=good, contribution_mask=bad)
        assert str(info.value) == CM.MASK_MSG
    with pytest.raises(Exception, match="pass contributions too"):
        _cpu_call(contribution_mask=torch.ones(4, 6))
    with pytest.raises(Exception) as info:
        _cpu_call(contributions=good, binning_capacity=100)
    assert str(info.value) == _C.CONTRIB_CAPACITY_MSG
    assert fake_native["forward"] == 0 and not fake_native["contrib"] and good.views == 0   # nothing was rendered
    # well-formed calls: the output tuple is what it was, the mask arrives as float32 [H * W], accumulate is on
    assert len(_cpu_call(contributions=good)) == 3 and good.views == 1
    out = _cpu_call(contributions=good, contribution_mask=torch.tensor([[True] * 6, [False] * 6] * 2), return_depth="distance",
                    colors_precomp2=torch.ones(5, 3))
    assert len(out) == 5 and float(out[-1][0, 0]) == 2.0 and good.views == 2
    _cpu_call(contributions=good, contribution_mask=torch.ones(1, 4, 6))
    a, b, c = fake_native["contrib"]
    assert (a["R"], a["P"], a["H"], a["W"], a["mask"], a["accumulate"]) == (7, 5, 4, 6, None, True)
    assert b["mask"].dtype == torch.float32 and b["mask"].shape == (24,) and b["mask"].tolist() == ([1.0] * 6 + [0.0] * 6) * 2
    assert c["mask"].shape == (24,) and bool(c["mask"].all())
    assert good.hits.tolist() == [3] * 5


def test_collect_contributions_feeds_the_first_call_of_the_block_only(fake_native):
    from diff_gaussian_rasterization import ContributionStats, collect_contributions, contributions as CM
    a, b = ContributionStats(5, "cpu"), ContributionStats(5, "cpu")
    _cpu_call()
    assert not fake_native["contrib"]
    mask = torch.ones(4, 6)
    with collect_contributions(a, mask) as got:
        assert got is a
        _cpu_call()
        _cpu_call()          # the second and third call of the block (a depth render, a second tone) are not fed
        _cpu_call()
    assert a.views == 1 and len(fake_native["contrib"]) == 1 and fake_native["contrib"][0]["mask"] is not None
    _cpu_call()
    assert a.views == 1 and len(fake_native["contrib"]) == 1    # the block is closed
    # nesting: the inner block feeds its own first call, the outer one is still waiting for its first afterwards
    with collect_contributions(a):
        with collect_contributions(b):
            _cpu_call()
            _cpu_call()
        assert (a.views, b.views) == (1, 1)
        _cpu_call()
        _cpu_call()
    assert (a.views, b.views) == (2, 1)
    # an explicit keyword inside a block does not consume the block's
    with collect_contributions(a):
        _cpu_call(contributions=b)
        assert (a.views, b.views) == (2, 2)
        _cpu_call()
    assert (a.views, b.views) == (3, 2)
    # a call refused before it rendered hands the pending statistics back
    with collect_contributions(a):
        with pytest.raises(Exception):
            _cpu_call(binning_capacity=100)
        _cpu_call()
    assert a.views == 4
    # restored after an exception, and thread-local
    with pytest.raises(KeyError):
        with collect_contributions(a):
            raise KeyError("x")
    assert CM.take_pending() == (None, None)
    seen = []
    with collect_contributions(a):
        t = threading.Thread(target=lambda: seen.append(CM.take_pending()))
        t.start()
        t.join()
        assert CM.take_pending()[0] is a
    assert seen == [(None, None)]
    with pytest.raises(Exception) as info:
        with collect_contributions(torch.zeros(5)):
            pass
    assert str(info.value) == CM.STATS_MSG


def test_contribution_stats_arithmetic():
    from diff_gaussian_rasterization import ContributionStats
    s = ContributionStats(4, "cpu")
    assert s.max_weight.dtype == torch.float32 and s.hits.dtype == torch.int64 and s.weight_sum_q32.dtype == torch.int64
    assert s.max_weight.shape == s.hits.shape == s.weight_sum_q32.shape == (4,) and s.views == 0 and s.P == 4
    assert bool(s.keep_mask().all())
    s.max_weight.copy_(torch.tensor([0.0, 0.01, 0.5, float("nan")]))
    s.hits.copy_(torch.tensor([0, 3, 900, 1]))
    s.weight_sum_q32.copy_(torch.tensor([0, 1 << 26, 300 << 32, (1 << 32) + 1]))
    s.views = 2
    ws = s.weight_sum
    assert ws.dtype == torch.float64 and ws.tolist() == [0.0, 2.0 ** -6, 300.0, 1.0 + 2.0 ** -32]
    assert s.keep_mask(min_hits=1).tolist() == [False, True, True, True]
    assert s.keep_mask(min_max_weight=0.1).tolist() == [False, False, True, True]     # a NaN maximum is kept
    assert s.keep_mask(min_weight_sum=1.0).tolist() == [False, False, True, True]
    assert s.keep_mask(min_hits=2, min_weight_sum=1.0).tolist() == [False, False, True, False]
    assert s.keep_mask(min_max_weight=0.0, min_hits=0, min_weight_sum=0.0).tolist() == [True] * 4
    o = ContributionStats(4, "cpu")
    o.max_weight.copy_(torch.tensor([0.2, 0.005, 0.7, 0.1]))
    o.hits.copy_(torch.tensor([5, 0, 1, 1]))
    o.weight_sum_q32.copy_(torch.tensor([7, 0, 1, 2]))
    o.views = 3
    assert s.merge_(o) is s and s.views == 5
    assert s.hits.tolist() == [5, 3, 901, 2] and s.weight_sum_q32.tolist() == [7, 1 << 26, (300 << 32) + 1, (1 << 32) + 3]
    assert torch.equal(s.max_weight[:3], torch.tensor([0.2, 0.01, 0.7])) and bool(torch.isnan(s.max_weight[3]))
    with pytest.raises(ValueError):
        s.merge_(ContributionStats(3, "cpu"))
    assert s.reset() is s and s.views == 0 and not s.hits.any() and not s.weight_sum_q32.any() and not s.max_weight.any()
    with pytest.raises(ValueError):
        ContributionStats(-1, "cpu")


def test_sweep_and_prune_helpers_without_a_device(fake_native):
    import wg_integration
    from diff_gaussian_rasterization import ContributionStats

    class Model:
        def __init__(self):
            self.xyz = torch.zeros(5, 3)
            self.pruned = None

        def _prune_points(self, mask):
            self.pruned = mask.clone()

    class Trainer:
        def __init__(self):
            self.model = Model()
            self.rendered = []

        def render(self, camera):
            assert not torch.is_grad_enabled()
            self.rendered.append(camera)
            _cpu_call()
            _cpu_call()   # a second rasterizer call over the same geometry
    t = Trainer()
    stats = wg_integration.contribution_sweep(t, ["a", "b", "c"], masks=[None, torch.ones(4, 6), np.ones((4, 6), np.float32)])
    assert isinstance(stats, ContributionStats) and stats.views == 3 and t.rendered == ["a", "b", "c"]
    assert stats.hits.tolist() == [3] * 5 and [c["mask"] is None for c in fake_native["contrib"]] == [True, False, False]
    with pytest.raises(ValueError):
        wg_integration.contribution_sweep(t, ["a"], masks=[None, None])
    assert wg_integration.prune_by_contribution(t, ["a", "b"], min_hits=1) == 0 and t.model.pruned is None
    assert wg_integration.prune_by_contribution(t, ["a", "b"], min_hits=3) == 5 and bool(t.model.pruned.all())
    with pytest.raises(ValueError):
        wg_integration.prune_by_contribution(t, ["a"])

    class Silent(Trainer):
        def render(self, camera):
            pass
    with pytest.raises(RuntimeError, match="frames were collected"):
        wg_integration.contribution_sweep(Silent(), ["a"])


def test_the_ctypes_struct_has_the_headers_fields_and_size():
    """_abi.py's _ContribArgs against include/wg_rasterizer.h: the same field names in the same order, and the size the header's types give
    under natural alignment (size_t and pointers 8 bytes, int 4)."""
    from diff_gaussian_rasterization._abi import _ContribArgs
    text = open(os.path.join(ROOT, "include", "wg_rasterizer.h")).read()
    body = re.search(r"typedef struct wg_contrib_args \{(.*?)\} wg_contrib_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "," in decl:   # "char *a, *b, *c" / "int P, R, width, height"
            first, rest = decl.split(",", 1)
            m = re.match(r"(.*?)([\*\s]+)(\w+)$", first.strip())
            base = m.group(1).strip()
            names = [m.group(2).strip() + m.group(3)] + [n.strip() for n in rest.split(",")]
        else:
            m = re.match(r"(.*?)([\*\s]+)(\w+)$", decl)
            base, names = m.group(1).strip(), [m.group(2).strip() + m.group(3)]
        for n in names:
            pointer = n.startswith("*")
            size = 8 if pointer or base == "size_t" else {"int": 4, "float": 4}[base]
            fields.append((n.lstrip("*"), size))
    assert [n for n, _ in fields] == [n for n, _ in _ContribArgs._fields_]
    assert [n for n, _ in fields] == ["struct_size", "P", "R", "width", "height", "geom_buffer", "binning_buffer", "image_buffer", "subpixel_offset",
                                     "pixel_mask", "options", "max_weight", "hits", "weight_sum_q32", "accumulate", "debug", "stream"]
    offset = 0
    for _n, size in fields:
        offset = (offset + size - 1) // size * size + size
    total = (offset + 7) // 8 * 8
    assert C.sizeof(_ContribArgs) == total == 112
    for (n, size), (cn, ctype) in zip(fields, _ContribArgs._fields_):
        assert C.sizeof(ctype) == size, n


def test_the_library_exports_the_call_and_names_the_stage():
    from diff_gaussian_rasterization import _abi
    path = os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so")
    lib = C.CDLL(path)
    assert hasattr(lib, "wg_render_contributions")
    lib.wg_render_contributions.restype = C.c_int
    lib.wg_render_contributions.argtypes = [C.POINTER(_abi._ContribArgs)]
    assert lib.wg_render_contributions(None) == -1
    a = _abi._ContribArgs()
    a.struct_size = C.sizeof(a) - 8
    assert lib.wg_render_contributions(C.byref(a)) == -1      # a shorter struct: refused before any device work
    a.struct_size = C.sizeof(a)
    a.width = a.height = 4
    assert lib.wg_render_contributions(C.byref(a)) == -1      # all three outputs NULL
    lib.wg_stage_name.restype = C.c_char_p
    names = [lib.wg_stage_name(i).decode() for i in range(12)]
    assert names[-1] == "render_contributions" and names[-2] == "render_depth_backward" and lib.wg_stage_name(12).decode() == "?"
    lib.wg_get_option.argtypes = [C.c_char_p]
    assert lib.wg_get_option(b"contribution_calls") >= 0      # (-1: an unknown name)
    assert lib.wg_get_option(b"contribution_call") == -1
    lib.wg_set_option.argtypes = [C.c_char_p, C.c_int]
    assert lib.wg_set_option(b"contribution_calls", 1) != 0   # read-only
