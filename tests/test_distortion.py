"""The distortion pass (wg_render_distortion / wg_distortion_grad; csrc/distortion/distortion.hip, distortion_bwd.hip):
`GaussianRasterizer.forward(..., return_distortion=, distortion_grad=)` returns dist[pixel] = sum_{j<i} w_i w_j (v_i - v_j)^2 of the frame's own
blend weights, from moments centred on each pixel's first blended v, and makes it differentiable in one more per-tile walk of the backward call.

Yardsticks (tests/distortion_lib.py; none runs the code under test): Y-w, the operator's one-hot-colour calls, exact weights, the pair sum in
float64; Y-32 / Y-64, the (1, v, v^2) route through the operator, the float32 oracle and the float64 oracle.
Bars: the centred bound (2n + 3) 2^-24 (A S2 + S1^2) against Y-w (derived in distortion_lib.centred_bound); the uncentred bound of
test_multi_tile_maps_match_the_float32_composition; GRAD_BAR = 1e-3 against the float32 oracle's route; against the float64 oracle's at most
twice the operator's own route's error; ORDER_BAR = 2e-6 between two orders of the same float32 sums.

Observed on an MI355X (profiles/distortion/accuracy.json has every figure; the docstrings below quote the largest): gradients within 2.4e-6 of
the float32 oracle's route; against the float64 oracle's at most 1.8e-4, at most 1.05 x the operator's own route's error."""
import ctypes as C
import glob
import inspect
import json
import os

import numpy as np
import pytest
import torch

import wg_scenes as S
import distortion_lib as L
from distortion_lib import BG, EPS, GEOMETRY, GRAD_BAR, ORDER_BAR
from wg_testlib import make_settings, rel_err, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
BINDINGS = ["torch", "ctypes"]


def _record(key, value):
    """profiles/distortion/accuracy.json, written only when asked for (WG_WRITE_PROFILES=1)"""
    if os.environ.get("WG_WRITE_PROFILES") != "1":
        return
    path = os.path.join(ROOT, "profiles", "distortion", "accuracy.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


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
    set_(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, staged_scatter=-1, force_global_sort=0, geometry_reuse=_C.GEOMETRY_REUSE_DEFAULT)


def _counters():
    from diff_gaussian_rasterization import _C
    return _C.get_option("distortion_calls"), _C.get_option("distortion_grad_calls")


def _oracle(oracle, name, precision):
    """(the image call's gradients, the route's) of a scene, computed once"""
    sc = L.scene(name)
    return (L.cached(("oracle-image", name, precision), lambda: L.oracle_image_call(oracle, sc, precision)),
            L.cached(("oracle-route", name, precision), lambda: L.oracle_route(oracle, sc, precision)))


def _oracle_sum(oracle, name, mode, image, precision):
    one, two = _oracle(oracle, name, precision)
    return L.sum_routes(L.scene(name), one, two, mode, image)


# ---- 0. the condition on the scenes (no device) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.SCENES))
def test_the_float32_oracles_route_lies_within_the_bar_of_the_float64_one(oracle, name):
    """The premise of the gradient tests: on each scene the float32 oracle's (1, v, v^2) route is itself within 2.5e-4 of the float64 oracle's."""
    for mode in ("values", "distance"):
        for image in (True, False):
            e = L.errors(_oracle_sum(oracle, name, mode, image, "f32"), _oracle_sum(oracle, name, mode, image, "f64"), mode)
            assert max(e.values()) <= L.ROUTE_BAR, (name, mode, image, e)


# ---- 1. the forward map on one-tile scenes --------------------------------------------------------------------------------------------------
def _yw(P, exact, v=None, tag=None):
    sc = L.one_tile(P, v)
    return sc, L.cached(("yw", P, exact, tag), lambda: L.exact_distortion(L.exact_weights(sc, exact), sc["v"], L.tile_order(sc, exact)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BINDINGS)
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 129, 200])
def test_one_tile_maps_match_the_exact_weights(binding, P, exact, name):
    """Values mode (v = the float32 distances torch.norm gives) is held to the centred bound.  Distance mode computes v in the kernel,
    sqrtf(dx dx + dy dy + dz dz) under contraction, which may differ from torch.norm's float32 by the roundings of either: three products, two
    additions and a square root on each side, at most 4 eps v between them.  d dist / d v_i = 2 w_i (A u_i - D'), so that adds at most
    sum_i 2 w_i (A |u_i| + S1) 4 eps vmax = 16 eps vmax A S1 to the bound there.
    Observed: the largest ratio of |map - Y-w| to the bound over all cases is 0.23 (P = 2, values mode; 0.03 to 0.06 from P = 63 on; at most
    0.055 in distance mode)."""
    assert built or name == "ctypes"
    binding.use_binding(name)
    sc, y = _yw(P, exact)
    for mode in ("values", "distance"):
        got = L.forward_map(sc, mode, exact)
        if P == 1:
            assert torch.equal(got, torch.zeros_like(got))
            continue
        err = np.abs(got.double().cpu().numpy() - y["dist"])
        bound = L.centred_bound(y)
        if mode == "distance":
            bound = bound + 16.0 * EPS * float(sc["v"].max()) * y["A"] * y["S1"]
        assert float(y["dist"].max()) > 0 and bound.min() > 0
        ratio = float((err / bound).max())
        print(f"one tile, P = {P}, exact={exact}, {name}, {mode}: largest |map - Y-w| / bound = {ratio:.3f}")
        _record(f"one_tile/P={P}/exact={exact}/{name}/{mode}", dict(ratio_to_centred_bound=ratio, k=2 * y["n"] + 3))
        assert (err <= bound).all(), ratio


# ---- 2. a thin surface ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_thin_surface_far_away_is_no_worse_than_the_float32_composition():
    """one_tile(65) with v = 50 + 1e-3 uniform.  Observed: the new map's largest error 4.9e-14 of a largest value 1.9e-8 (ratio to the bound
    0.057); the float32 (1, v, v^2) composition's largest error on the same frame 5.5e-4 -- four orders above the value itself."""
    P = 65
    v = (50.0 + 1e-3 * np.random.default_rng(1).uniform(size=P)).astype(np.float32)
    sc, y = _yw(P, 1, v, "thin")
    got = L.forward_map(sc, "values", 1).double().cpu().numpy()
    err, bound = np.abs(got - y["dist"]), L.centred_bound(y)
    comp = L.operator_route(sc, backward=False)["dist32"].astype(np.float64)
    err_comp = np.abs(comp - y["dist"])
    print(f"thin surface: largest value {y['dist'].max():.3e}; new map: largest error {err.max():.3e}, ratio to the bound {(err / bound).max():.3f}; "
          f"float32 composition: largest error {err_comp.max():.3e}")
    _record("thin_surface", dict(largest_value=float(y["dist"].max()), new_map_max_err=float(err.max()), ratio_to_centred_bound=float((err / bound).max()),
                                 float32_composition_max_err=float(err_comp.max())))
    assert (err <= bound).all()
    assert err.max() <= err_comp.max()


# ---- 3. the forward map on multi-tile scenes ------------------------------------------------------------------------------------------------
def _longest_walk_and_range(sc, exact):
    """n = the longest walked list (max tile_last) and rho = vmax / vmin over the Gaussians that reach the image, from the frame itself"""
    from diff_gaussian_rasterization import _C
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    rs = L.settings(sc)
    e = torch.Tensor([])
    f = _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                               rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0, rs.campos, False, False,
                               options=dict(exact_compositing=int(bool(exact))))
    n = int(_C.view_image(f[5], rs.image_height, rs.image_width)["tile_last"].max())
    vis = (f[2] > 0).cpu().numpy()
    return n, float(sc["v"][vis].max() / sc["v"][vis].min())


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("mode", ["values", "distance"])
@pytest.mark.parametrize("name", list(L.SCENES))
def test_multi_tile_maps_match_the_float32_composition(name, mode, exact):
    """Against the operator's own float32 composition A * Q - D * D of its (1, v, v^2) render: the decisions are the same bit for bit, so no
    threshold can flip.  The bound is uncentred, k'(n) 2^-24 (A Q + D^2) with n the longest walked list:
      the composition: A carries (n - 1) eps, D n eps, Q (n + 1) eps (v^2 is rounded once more), A * Q and D * D one each, the subtraction one
      -> at most (2n + 3) eps (A Q + D^2);
      the new map: (2n + 3) eps (A S2 + S1^2) (distortion_lib.centred_bound).  With 0 < vmin <= v <= vmax over the Gaussians that reach the image
      and rho = vmax / vmin: c <= vmax and D >= A vmin give c A <= rho D, so S2 = Q - 2 c D + c^2 A <= Q + c^2 A and S1 <= D + c A, hence
      A S2 + S1^2 <= A Q + 2 D^2 + 3 c^2 A^2 <= (2 + 3 rho^2) (A Q + D^2);
      together k'(n) = (2n + 3) (3 + 3 rho^2).  Loose by construction -- what the uncentred route can resolve; the centred tests above are the sharp
      ones.  Observed: rho 11.2 to 12.4, n 81 to 195, the largest ratio to this bound 1.2e-4."""
    sc = L.scene(name)
    got = L.forward_map(sc, mode, exact)
    route = L.cached(("op-route-fwd", name, exact), lambda: L.operator_route(sc, exact, backward=False))
    n, rho = L.cached(("walk", name, exact), lambda: _longest_walk_and_range(sc, exact))
    A, D, Q = (route["image"][c].astype(np.float64) for c in range(3))
    bound = (2 * n + 3) * (3 + 3 * rho * rho) * EPS * (A * Q + D * D)
    err = np.abs(got.double().cpu().numpy() - route["dist32"].astype(np.float64))
    covered = bound > 0
    assert (err[~covered] == 0).all() and float(got.max()) > 0
    ratio = float((err[covered] / bound[covered]).max())
    print(f"{name} / {mode} / exact={exact}: n = {n}, rho = {rho:.2f}, largest |map - composition| / bound = {ratio:.3e}")
    _record(f"multi_tile/{name}/{mode}/exact={exact}", dict(n=n, rho=rho, ratio_to_uncentred_bound=ratio))
    assert ratio <= 1.0
    if mode == "values":   # a power of two scales every u, D', Q' exactly: 4 x the map, bit for bit
        assert torch.equal(L.forward_map(sc, "values", exact, v=2.0 * sc["v"]), 4.0 * got)
        assert torch.equal(L.forward_map(sc, "values", exact), got)   # and two calls give the same bits


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------------
def _new(name, mode, image, exact):
    return L.cached(("new", name, mode, image, exact), lambda: L.new_call(L.scene(name), mode, image, exact))


def _operator_sum(name, mode, image, exact=1):
    sc = L.scene(name)
    one = L.cached(("op-image", name, exact), lambda: L.operator_image_call(sc, exact)) if image else None
    two = L.cached(("op-route", name, exact), lambda: L.operator_route(sc, exact))["grads"]
    return L.sum_routes(sc, one, two, mode, image)


@pytest.mark.gpu
@pytest.mark.parametrize("image", [True, False], ids=["image+dist", "dist-only"])
@pytest.mark.parametrize("name", list(L.SCENES))
@pytest.mark.parametrize("mode", ["values", "distance"])
@pytest.mark.parametrize("exact", [1, 0])
def test_gradients_match_the_float32_oracles_route(oracle, exact, mode, name, image):
    before = _counters()
    got = L.new_call(L.scene(name), mode, image, exact)
    assert _counters() == (before[0] + 1, before[1] + 1)
    ref = _oracle_sum(oracle, name, mode, image, "f32")
    errs = L.errors(got["grads"], ref, mode)
    errs["means2D.z"] = rel_err(got["grads"]["means2D"][:, 2], ref["means2D"][:, 2])   # the abs term on its own scale
    for c in (0, 1):
        errs[f"means2D.{'xy'[c]}"] = rel_err(got["grads"]["means2D"][:, c], ref["means2D"][:, c])
    print(f"{name} / {mode} / exact={exact} / image={image}: rel_err against the float32 oracle's route: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    for k in GEOMETRY:
        assert np.abs(ref[k]).max() > 0, k
    for k, e in errs.items():
        assert e <= GRAD_BAR, (k, e)
    if mode == "distance":
        assert got["grads"]["values"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("image", [True, False], ids=["image+dist", "dist-only"])
@pytest.mark.parametrize("name", list(L.SCENES))
@pytest.mark.parametrize("mode", ["values", "distance"])
def test_error_against_float64_is_at_most_twice_the_operators_route(oracle, mode, name, image):
    ref = _oracle_sum(oracle, name, mode, image, "f64")
    e_new = L.errors(_new(name, mode, image, 1)["grads"], ref, mode)
    e_two = L.errors(_operator_sum(name, mode, image), ref, mode)
    print(f"{name} / {mode} / image={image}: rel_err against the float64 oracle, new path | the operator's route: " +
          ", ".join(f"{k} {e_new[k]:.3e} | {e_two[k]:.3e}" for k in e_new))
    _record(f"gradients/{name}/{mode}/{'image+dist' if image else 'dist-only'}",
            {k: dict(rel_err_f64_new_path=e_new[k], rel_err_f64_operator_route=e_two[k]) for k in e_new})
    for k in e_new:
        assert e_new[k] <= GRAD_BAR, (k, e_new[k])
        if e_two[k] > 0:
            assert e_new[k] <= 2 * e_two[k], (k, e_new[k], e_two[k])


# ---- 5. identities on the new path alone ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_value_gradients_sum_to_zero_and_reproduce_twice_the_map():
    """dist is invariant under a shift of v and homogeneous of degree 2 in it: sum_g dL/dv_g = 0 and sum_g v_g dL/dv_g = 2 <g, dist>.
    On one_tile(129), whose exact weights give the size of the terms 2 g w_i (A u_i - D') behind the sums: sum |terms| is taken as
    sum 2 |g| w_i (A |u_i| + S1) in float64.  A-priori count of float32 roundings behind one term's way into the total, n = 129 instances:
    the backward walk's T is rebuilt by n steps of three roundings (1 - alpha, its reciprocal, the product): 3n; A and D' carry n each: 2n;
    the term's own arithmetic: 8; the wave's reduction over 256 pixels: 256 -> (5n + 264) 2^-24 = 5.4e-5 relative to sum |terms|.
    Observed: 2.3e-8 and 7.6e-9."""
    P = 129
    sc, y = _yw(P, 1)
    got = L.new_call(sc, "values", False, 1)
    dv = got["grads"]["values"]
    w = L.exact_weights(sc, 1).double().cpu().numpy()
    order = L.tile_order(sc, 1)
    v = sc["v"].astype(np.float64)
    first = np.argmax(w[order] > 0, axis=0)
    u = np.abs(v[:, None, None] - v[order][first][None])
    g = np.abs(sc["cot_t"].astype(np.float64))
    size = 2.0 * g[None] * w * (y["A"][None] * u + y["S1"][None])        # [P, H, W]
    K = (5 * y["n"] + 264) * EPS
    r0 = abs(dv.sum()) / size.sum()
    lhs, rhs = float((v * dv).sum()), 2.0 * float((sc["cot_t"].astype(np.float64) * got["dist"].astype(np.float64)).sum())
    r1 = abs(lhs - rhs) / float((v[:, None, None] * size).sum())
    print(f"identities: |sum dL/dv| / sum|terms| = {r0:.3e}, |sum v dL/dv - 2 <g, dist>| / sum|v terms| = {r1:.3e}, bound {K:.3e}")
    _record("identities", dict(shift=float(r0), degree_two=float(r1), bound=K))
    assert abs(rhs) > 0 and r0 <= K and r1 <= K


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------------
def _against_route(sc, mode, image=True, exact=True, **fwd):
    got = L.new_call(sc, mode, image, exact, **fwd)
    ref = L.sum_routes(sc, L.operator_image_call(sc, exact) if image else None, L.operator_route(sc, exact)["grads"], mode, image)
    return L.errors(got["grads"], ref, mode), got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (17, 33)])
def test_small_and_ragged_images(size):
    W, H = size
    sc = L.with_cotangents(S.make_cloud(400, W, H, sh_degree=None, seed=2, scale_mult=20.0), S.make_camera(W, H))
    for mode in ("values", "distance"):
        errs, got, ref = _against_route(sc, mode)
        assert got["dist"].shape == (H, W) and np.abs(ref["values"]).max() > 0
        for k, e in errs.items():
            assert e <= GRAD_BAR, (mode, k, e)


@pytest.mark.gpu
def test_empty_frames_leave_zero_outputs_and_the_counters_alone():
    """P = 0; everything culled, which is R = 0: a zero map, zero gradients, no walk."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = L.scene("ragged")
    before = _counters()
    behind = dict(sc, cloud=dict(sc["cloud"], means3D=sc["cloud"]["means3D"] * np.array([1, 1, -1], np.float32)))
    for mode in ("values", "distance"):
        got = L.new_call(behind, mode)
        assert not got["dist"].any()
        for k in GEOMETRY + (("values",) if mode == "values" else ()):
            assert got["grads"][k] is not None and not got["grads"][k].any(), (mode, k)
    rs = make_settings(sc["cam"], 0)
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    for source in ("distance", z(0)):
        t = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
        out = GaussianRasterizer(rs)(**t, return_distortion=source, distortion_grad=True)
        assert not out[-1].any()
        (out[-1].sum() + out[0].sum()).backward()
        assert t["means3D"].grad is not None and t["means3D"].grad.shape == (0, 3)
    assert _counters() == before


@pytest.mark.gpu
def test_pixels_without_a_contributor_beside_pixels_that_stopped_early():
    sc = L.scene("saturating")
    keep = sc["cloud"]["means3D"][:, 0] > 0.15 * sc["cloud"]["means3D"][:, 2]
    half = L.with_cotangents({k: np.ascontiguousarray(a[keep]) for k, a in sc["cloud"].items()}, sc["cam"])
    errs, got, ref = _against_route(half, "values")
    assert int((got["dist"] == 0).sum()) > 1000 and int((got["dist"] > 0).sum()) > 1000
    for k, e in errs.items():
        assert e <= GRAD_BAR, (k, e)


@pytest.mark.gpu
def test_a_gaussian_at_distance_zero_gets_a_finite_gradient_and_no_direct_term():
    """campos put ON a visible Gaussian's mean (the view matrix stays): distance mode then equals values mode with v = torch.norm(means3D - campos)
    under autograd, whose subgradient at 0 is 0."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = L.scene("plain")
    dv_ref = L.cached(("op-route", "plain", 1), lambda: L.operator_route(sc, 1))["grads"]["values"]
    g = int(np.argmax(np.abs(dv_ref)))
    cam = dict(sc["cam"], campos=sc["cloud"]["means3D"][g].copy())
    rs = make_settings(cam, 0, bg=np.array(BG, np.float32))
    cot_t = to_dev(sc["cot_t"])
    grads = {}
    for mode in ("distance", "values"):
        t = L.leaves(sc)
        source = "distance" if mode == "distance" else torch.norm(t["means3D"] - rs.campos[None], dim=-1)
        if mode == "values":
            assert float(source[g]) == 0.0
        out = GaussianRasterizer(rs)(**L.geo(t), colors_precomp=t["colors_precomp"], return_distortion=source, distortion_grad=True)
        (out[-1] * cot_t).sum().backward()
        grads[mode] = L.grads(t)
    for k in GEOMETRY:
        assert np.isfinite(grads["distance"][k]).all(), k
        assert rel_err(grads["distance"][k], grads["values"][k]) <= GRAD_BAR, k
    scale = np.abs(grads["values"]["means3D"]).max()
    assert np.abs(grads["distance"]["means3D"][g] - grads["values"]["means3D"][g]).max() <= GRAD_BAR * scale


@pytest.mark.gpu
def test_a_nan_value_stays_with_the_gaussians_it_shares_a_pixel_with():
    """No claim beyond that: a Gaussian whose tile rectangle is disjoint from the NaN Gaussian's shares no pixel with it."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from wg_testlib import run_hip_native
    sc = L.scene("plain")
    n = run_hip_native(sc["cloud"], sc["cam"], sh_degree=0)
    sp = n["views"]["geometry"]["splats"].cpu().numpy()
    radii = n["radii"].cpu().numpy()
    mx, my = sp[:, 0], sp[:, 1]
    inside = (radii > 0) & (mx > 100) & (mx < 156) & (my > 100) & (my < 156)
    g = int(np.flatnonzero(inside)[0])
    far = (radii > 0) & ((np.abs(mx - mx[g]) > radii + radii[g] + 32) | (np.abs(my - my[g]) > radii + radii[g] + 32))
    assert int(far.sum()) > 1000
    t = L.leaves(sc)
    values = to_dev(sc["v"]).clone()
    values[g] = float("nan")
    values.requires_grad_(True)
    out = GaussianRasterizer(L.settings(sc))(**L.geo(t), colors_precomp=t["colors_precomp"], return_distortion=values, distortion_grad=True)
    assert bool(torch.isnan(out[-1]).any()) and bool(torch.isfinite(out[-1]).any())
    ((out[-1].nan_to_num() * to_dev(sc["cot_t"])).sum() + (out[0] * to_dev(sc["cot"])).sum()).backward()
    far_t = torch.from_numpy(far).cuda()
    for k in GEOMETRY:
        assert torch.isfinite(t[k].grad[far_t]).all(), k
    assert torch.isfinite(values.grad[far_t]).all()


# ---- 7. binning paths -----------------------------------------------------------------------------------------------------------------------
PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["saturating", "dense"])
def test_every_binning_path_gives_the_same_map_and_gradients(options, name, path):
    """The walks read each tile's list up to tile_last only: behind it lie the unsorted tails of lazily sorted lists."""
    sc = L.scene(name)
    base = L.cached(("path-default", name), lambda: L.new_call(sc, "distance"))
    options(**PATHS[path])
    got = L.new_call(sc, "distance")
    assert np.array_equal(got["dist"], base["dist"])
    for k in GEOMETRY:
        e = rel_err(got["grads"][k], base["grads"][k])
        print(f"{name} / {path}: {k} rel_err against the default path = {e:.3e}")
        assert e <= ORDER_BAR, (k, e)


# ---- 8. colour sources ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_colour_source_of_the_call():
    """SH colours (the backward-row kernel), a tone, raw parameters: the geometry gradients are the image call's plus the route's at the 1e-3
    bar, and the colours' own gradients come out as without the keyword."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    P, W, H = 3000, 160, 96
    cam = S.make_camera(W, H)
    sc = L.with_cotangents(S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=3.0), cam)
    shs0 = S.make_cloud(P, W, H, sh_degree=1, seed=3, scale_mult=3.0)["shs"]
    rs, rs0 = make_settings(cam, 1, bg=np.array(BG, np.float32)), make_settings(cam, 1)
    cot, cot_t, v = to_dev(sc["cot"]), to_dev(sc["cot_t"]), to_dev(sc["v"])
    ones = torch.ones(P, 3, device="cuda")
    f3d = torch.full((P, 1), 0.01, device="cuda")

    def leaves(raw):
        t = L.leaves(sc)
        if raw:
            t["opacities"] = torch.logit(t["opacities"].detach().clamp(0.01, 0.99)).requires_grad_(True)
            t["scales"] = torch.log(t["scales"].detach()).requires_grad_(True)
        t["shs"] = to_dev(shs0).requires_grad_(True)
        t["mul"], t["offset"] = (0.5 * ones).requires_grad_(True), (0.1 * ones).requires_grad_(True)
        return t
    sources = dict(
        shs=lambda t: dict(shs=t["shs"]),
        tone=lambda t: dict(shs=t["shs"], sh_mul=t["mul"], sh_offset=t["offset"], sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0),
        raw=lambda t: dict(colors_precomp=t["colors_precomp"], filter_3D=f3d))
    colour_leaves = ("shs", "colors_precomp", "mul", "offset")
    rows_before = _C.get_option("backward_row_calls")
    for name, make in sources.items():
        raw = name == "raw"
        extra = dict(filter_3D=f3d) if raw else {}
        t1 = leaves(raw)   # (i) the same call without the keyword
        (GaussianRasterizer(rs)(**L.geo(t1), **make(t1))[0] * cot).sum().backward()
        t2 = leaves(raw)   # (ii) the (1, v, v^2) route
        colors = to_dev(L.moment_colours(sc["v"])).requires_grad_(True)
        out2 = GaussianRasterizer(rs0)(**L.geo(t2), colors_precomp=colors, **extra)
        out2[0].backward(torch.from_numpy(L.route_cotangent(out2[0].detach().cpu().numpy(), sc["cot_t"]).astype(np.float32)).cuda())
        dv_ref = L.values_gradient(colors.grad.cpu().numpy(), sc["v"])
        t3 = leaves(raw)   # the new path
        values = v.clone().requires_grad_(True)
        before = _counters()
        out = GaussianRasterizer(rs)(**L.geo(t3), **make(t3), return_distortion=values, distortion_grad=True)
        ((out[0] * cot).sum() + (out[-1] * cot_t).sum()).backward()
        assert _counters() == (before[0] + 1, before[1] + 1), name
        for k in GEOMETRY:
            ref = t1[k].grad.double() + t2[k].grad.double()
            e = rel_err(t3[k].grad.cpu().numpy(), ref.cpu().numpy())
            print(f"{name}: {k} rel_err against the sum of the calls = {e:.3e}")
            assert e <= GRAD_BAR, (name, k, e)
        assert rel_err(values.grad.cpu().numpy(), dv_ref) <= GRAD_BAR, name
        seen = 0
        for k in colour_leaves:
            assert (t1[k].grad is None) == (t3[k].grad is None), (name, k)
            if t1[k].grad is not None:
                seen += 1
                assert rel_err(t3[k].grad.cpu().numpy(), t1[k].grad.cpu().numpy()) <= ORDER_BAR, (name, k)
        assert seen >= 1, name
    assert _C.get_option("backward_row_calls") > rows_before


# ---- 9. beside depth in one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["values", "distance"])
def test_beside_the_depth_pass_in_one_call(mode):
    """return_depth + depth_grad and return_distortion + distortion_grad together: (color, radii, accumulation, depth, distortion); each gradient
    is the sum of the three routes -- the image call, depth's three-channel call (tests/test_render_depth_grad.py) and the (1, v, v^2) route --
    and one tensor feeding both takes the sum of both gradients."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    sc = L.scene("ragged")
    rs = L.settings(sc)
    cot, cot_t = to_dev(sc["cot"]), to_dev(sc["cot_t"])
    cot_d = torch.flip(cot_t, dims=(0,)).contiguous()   # a depth cotangent of its own
    t = L.leaves(sc)
    values = to_dev(sc["v"]).requires_grad_(True) if mode == "values" else None
    source = "distance" if values is None else values
    walks = _C.get_option("depth_grad_calls"), _counters()[1]
    out = GaussianRasterizer(rs)(**L.geo(t), colors_precomp=t["colors_precomp"], return_depth=source, depth_grad=True, return_distortion=source,
                                 distortion_grad=True)
    assert len(out) == 5 and out[3].shape == out[4].shape == (130, 250) and out[3].requires_grad and out[4].requires_grad
    assert torch.equal(out[4], L.forward_map(sc, mode))
    ((out[0] * cot).sum() + (out[3] * cot_d).sum() + (out[4] * cot_t).sum()).backward()
    assert (_C.get_option("depth_grad_calls"), _counters()[1]) == (walks[0] + 1, walks[1] + 1)
    # depth's route: colors = v repeated over a zero background under (cot_d, 0, 0)
    t2 = L.leaves(sc)
    colors = to_dev(sc["v"])[:, None].repeat(1, 3).requires_grad_(True)
    cot3 = torch.zeros_like(cot)
    cot3[0] = cot_d
    GaussianRasterizer(make_settings(sc["cam"], 0, subpixel_offset=sc["so"]))(**L.geo(t2), colors_precomp=colors)[0].backward(cot3)
    depth_route = L.grads(t2, values=colors.grad[:, 0].double().cpu().numpy())
    ref = _operator_sum("ragged", "values", True)   # (the direct terms are added below, for both)
    for k in GEOMETRY:
        ref[k] = ref[k] + depth_route[k]
    ref["values"] = ref["values"] + depth_route["values"]
    if mode == "distance":
        ref["means3D"] = ref["means3D"] + L.direct_term(sc, ref["values"])
    got = L.grads(t, values=None if values is None else values.grad.double().cpu().numpy())
    for k, e in L.errors(got, ref, mode).items():
        print(f"beside depth, {mode}: {k} rel_err against the three routes = {e:.3e}")
        assert e <= GRAD_BAR, (k, e)


# ---- 10. nothing moves without it -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_loss_without_the_map_is_the_call_without_the_keyword():
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = L.scene("ragged")
    rs = L.settings(sc)
    base = L.cached(("op-image", "ragged", 1), lambda: L.operator_image_call(sc, 1))
    before = _counters()
    t = L.leaves(sc)
    out = GaussianRasterizer(rs)(**L.geo(t), colors_precomp=t["colors_precomp"], return_distortion="distance", distortion_grad=True)
    assert out[-1].requires_grad
    out[0].backward(to_dev(sc["cot"]))   # the map takes no cotangent: None reaches the backward call
    got = L.grads(t)
    assert _counters() == (before[0] + 1, before[1])
    for k in GEOMETRY + ("colors_precomp",):
        assert rel_err(got[k], base[k]) <= ORDER_BAR, k
    for kw in (dict(distortion_grad=False), dict()):
        t = L.leaves(sc)
        out = GaussianRasterizer(rs)(**L.geo(t), colors_precomp=t["colors_precomp"], return_distortion="distance", **kw)
        assert len(out) == 4 and out[0].requires_grad and not out[-1].requires_grad
        out[0].backward(to_dev(sc["cot"]))
        for k in GEOMETRY:
            assert rel_err(L.grads(t)[k], base[k]) <= ORDER_BAR, k
    assert _counters()[1] == before[1]


# ---- 11. the C-ABI and both bindings --------------------------------------------------------------------------------------------------------
def _native_frame(_C, rs, t, **fwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                  rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0, rs.campos, False, False, **fwd)


def _native_backward(_C, rs, t, frame, dL, **bwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians_backward(rs.bg, t["means3D"], frame[2], t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                           rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, dL, e, 0, rs.campos,
                                           frame[3], frame[0], frame[4], frame[5], False, **bwd)


def _native_distortion(_C, rs, P, frame, source, t, **kw):
    return _C.render_distortion(frame[3], frame[4], frame[5], frame[0], P, rs.image_height, rs.image_width, source, means3D=t["means3D"], campos=rs.campos,
                                subpixel_offset=rs.subpixel_offset, **kw)


NATIVE_NAMES = ("means2D", "colors_precomp", "opacities", "means3D", "cov3Ds_precomp", "sh", "scales", "rotations")


@pytest.mark.gpu
def test_native_calls_and_refusals_under_both_bindings(binding):
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    sc = L.scene("ragged")
    P, H, W = sc["cloud"]["means3D"].shape[0], 130, 250
    rs = L.settings(sc)
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    dL, dLt, v = to_dev(sc["cot"]), to_dev(sc["cot_t"]), to_dev(sc["v"])
    want = {m: _operator_sum("ragged", m, True) for m in ("values", "distance")}
    geo = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
               colors_precomp=t["colors_precomp"])
    bad_mode = {"deterministic_backward": dict(options=dict(deterministic_backward=1)), "grad_record": dict(options=dict(grad_record=0)),
                "colour_gradients_only": dict(colour_gradients_only=True), "fixed_order": dict(colour_gradients_only="fixed_order")}
    bad_operator = {"deterministic_backward": dict(deterministic_backward=True), "grad_record": dict(grad_record=False),
                    "colour_gradients_only": dict(colour_gradients_only=True), "binning_capacity": dict(binning_capacity=1_000_000)}
    said, results = {}, {}
    for name in BINDINGS:
        _C.use_binding(name)
        frame = _native_frame(_C, rs, t)
        dist, mom = _native_distortion(_C, rs, P, frame, v, t, moments=True)
        assert dist.shape == (H, W) and mom.shape == (4, H, W)
        assert torch.equal(_native_distortion(_C, rs, P, frame, v, t), dist)   # without the moments: the same map
        before = _counters()
        bad_block = {"not a triple": (dLt, mom), "cotangent size": (dLt[:-1], mom, v), "cotangent dtype": (dLt.double(), mom, v),
                     "cotangent host": (dLt.cpu(), mom, v), "moments size": (dLt, mom[:3], v), "moments dtype": (dLt, mom.double(), v),
                     "moments host": (dLt, mom.cpu(), v), "values size": (dLt, mom, v[:-1]), "values dtype": (dLt, mom, v.double()),
                     "values host": (dLt, mom, v.cpu())}
        for case, block in bad_block.items():
            with pytest.raises(RuntimeError) as info:
                _native_backward(_C, rs, t, frame, dL, distortion=block)
            said[name, "block", case] = str(info.value)
        with pytest.raises(ValueError) as info:
            _native_backward(_C, rs, t, frame, dL, distortion=(dLt, mom, "nearest"))
        said[name, "block", "string"] = str(info.value)
        for case, kw in bad_mode.items():
            with pytest.raises(RuntimeError) as info:
                _native_backward(_C, rs, t, frame, dL, distortion=(dLt, mom, v), **kw)
            said[name, "mode", case] = str(info.value)
        for case, kw in bad_operator.items():
            for source in ("distance", v):
                with pytest.raises(Exception) as info:
                    GaussianRasterizer(rs)(**geo, return_distortion=source, distortion_grad=True, **kw)
                said[name, "operator", case, isinstance(source, str)] = str(info.value)
        for source in ("distance", v):
            with pytest.raises(Exception) as info:
                GaussianRasterizer(rs)(**geo, return_distortion=source, binning_capacity=1_000_000)
            said[name, "capacity", isinstance(source, str)] = str(info.value)
        for bad, exc in ((v[:-1], RuntimeError), (v.double(), RuntimeError), (v.cpu(), RuntimeError), ("nearest", ValueError)):
            with pytest.raises(exc):
                GaussianRasterizer(rs)(**geo, return_distortion=bad)
            with pytest.raises(exc):
                _native_distortion(_C, rs, P, frame, bad, t)
        with pytest.raises(Exception, match="pass return_distortion too"):
            GaussianRasterizer(rs)(**geo, distortion_grad=True)
        assert _counters() == before   # nothing was launched
        for mode, source in (("values", v), ("distance", "distance")):
            d2, m2 = _native_distortion(_C, rs, P, frame, source, t, moments=True)
            res = _native_backward(_C, rs, t, frame, dL, distortion=(dLt, m2, source))
            assert len(res) == 9 and res[8].shape == (P,) and res[8].dtype == torch.float32
            got = {k: r.double().cpu().numpy().reshape(P, -1) for k, r in zip(NATIVE_NAMES, res[:8]) if k in GEOMETRY}
            got["values"] = res[8].double().cpu().numpy()
            for k in GEOMETRY + ("values",):
                assert rel_err(got[k].reshape(want[mode][k].shape), want[mode][k]) <= GRAD_BAR, (name, mode, k)
            results[name, mode] = got
            # with the depth block too: ten, the distortion's dL_dvalues in front of depth's, which stays last
            both = _native_backward(_C, rs, t, frame, dL, distortion=(dLt, m2, source), depth=(torch.zeros_like(dLt), source))
            assert len(both) == 10 and not both[9].any() and rel_err(both[8].cpu().numpy(), res[8].cpu().numpy()) <= ORDER_BAR
        assert _counters() == (before[0] + 2, before[1] + 4)
        assert len(_native_backward(_C, rs, t, frame, dL)) == 8 and len(_native_backward(_C, rs, t, frame, dL, distortion=None)) == 8
        assert _counters()[1] == before[1] + 4
    for key in [k[1:] for k in said if k[0] == "torch"]:
        assert said[("torch",) + key] == said[("ctypes",) + key], key
    assert said["torch", "block", "not a triple"] == _C.DISTORTION_GRAD_BLOCK_MSG
    assert {said["torch", "block", c] for c in ("cotangent size", "cotangent dtype", "cotangent host")} == {_C.DISTORTION_GRAD_COTANGENT_MSG}
    assert {said["torch", "block", c] for c in ("moments size", "moments dtype", "moments host")} == {_C.DISTORTION_GRAD_MOMENTS_MSG}
    assert said["torch", "block", "values size"] == "distortion values must have P elements"
    assert {said["torch", "block", c] for c in ("values dtype", "values host", "string")} == {_C.DISTORTION_SOURCE_MSG}
    assert {said["torch", "mode", c] for c in bad_mode} == {_C.DISTORTION_GRAD_MSG}
    assert {m for k, m in said.items() if k[0] == "torch" and k[1] == "operator"} == {_C.DISTORTION_GRAD_MSG}
    assert {m for k, m in said.items() if k[0] == "torch" and k[1] == "capacity"} == {_C.DISTORTION_CAPACITY_MSG}
    for mode in ("values", "distance"):
        for k in GEOMETRY + ("values",):
            assert rel_err(results["torch", mode][k], results["ctypes", mode][k]) <= ORDER_BAR, (mode, k)


@pytest.mark.gpu
def test_c_abi_symbols_struct_sizes_guard_words_and_refusals():
    """wg_render_distortion and wg_rasterize_backward_with called directly: the outputs inside larger buffers whose guard words must survive, full
    of NaN on entry ("fully overwritten"); every refusal is WG_ERR_INVALID_ARGUMENT and writes nothing; a NULL extras, or a NULL block, is
    wg_rasterize_backward_ex."""
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _BackwardArgs, _BackwardExtras, _CallOptions, _DepthGrad, _DistortionArgs, _DistortionGrad
    lib = _C._lib
    assert hasattr(lib, "wg_render_distortion") and hasattr(lib, "wg_rasterize_backward_with")
    sizes = dict(wg_distortion_args=C.sizeof(_DistortionArgs), wg_distortion_grad=C.sizeof(_DistortionGrad), wg_backward_extras=C.sizeof(_BackwardExtras),
                 pointer=C.sizeof(C.c_void_p), size_t=C.sizeof(C.c_size_t), int=C.sizeof(C.c_int))
    _record("struct_sizes", sizes)
    assert sizes["wg_distortion_grad"] == 40 and sizes["wg_backward_extras"] == 16 and sizes["wg_distortion_args"] == 120
    assert C.sizeof(_BackwardArgs) == 328 and C.sizeof(_DepthGrad) == 32
    assert _C.STAGE_COUNT == 12 and lib.wg_stage_name(12) == b"?" and lib.wg_stage_name(11) != b"?"
    sc = L.scene("ragged")
    P, H, W = sc["cloud"]["means3D"].shape[0], 130, 250
    rs = L.settings(sc)
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    frame = _native_frame(_C, rs, t)
    dL, dLt, v = to_dev(sc["cot"]), to_dev(sc["cot_t"]), to_dev(sc["v"])
    G, N = 64, H * W
    dbuf, mbuf, vbuf = (torch.empty(G + n + G, device="cuda") for n in (N, 4 * N, P))
    outs = {k: torch.full((P, n), float("nan"), device="cuda") for k, n in (("mean2D", 3), ("opacity", 1), ("color", 3), ("mean3D", 3), ("scale", 3), ("rot", 4))}
    radii = frame[2].contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def fresh():
        for b in (dbuf, mbuf, vbuf):
            b.fill_(float("nan"))
            b[:G] = 7.0
            b[-G:] = 9.0
        for o in outs.values():
            o.fill_(float("nan"))

    def guards_ok():
        return all(bool((b[:G] == 7.0).all()) and bool((b[-G:] == 9.0).all()) for b in (dbuf, mbuf, vbuf))

    def fargs(options=None, **kw):
        a = _DistortionArgs()
        a.struct_size = C.sizeof(a)
        a.P, a.R, a.width, a.height = P, int(frame[0]), W, H
        a.geom_buffer, a.binning_buffer, a.image_buffer = frame[3].data_ptr(), frame[4].data_ptr(), frame[5].data_ptr()
        a.subpixel_offset, a.values, a.means3D, a.campos = rs.subpixel_offset.data_ptr(), v.data_ptr(), t["means3D"].data_ptr(), rs.campos.data_ptr()
        a.out_distortion, a.out_moments, a.stream = dbuf[G:].data_ptr(), mbuf[G:].data_ptr(), stream
        if options is not None:
            a.options = C.pointer(options)
        for k, val in kw.items():
            setattr(a, k, val)
        return a
    fwd = lambda a: lib.wg_render_distortion(C.byref(a))
    fresh()
    before = _counters()
    for i, a in enumerate([fargs(struct_size=112), fargs(out_distortion=None), fargs(values=None, campos=None), fargs(values=None, means3D=None),
                           fargs(P=-1), fargs(width=0), fargs(geom_buffer=None), fargs(_CallOptions(0, 0, 1))]):   # (the last: the frame is exact)
        assert fwd(a) == -1, i
    torch.cuda.synchronize()
    assert torch.isnan(dbuf[G:G + N]).all() and torch.isnan(mbuf[G:G + 4 * N]).all() and _counters() == before
    assert fwd(fargs()) == 0
    torch.cuda.synchronize()
    assert guards_ok() and torch.isfinite(dbuf).all() and torch.isfinite(mbuf).all()
    dist, mom = dbuf[G:G + N].clone().view(H, W), mbuf[G:G + 4 * N].clone()
    assert torch.equal(dist, L.forward_map(sc, "values"))
    fresh()
    assert fwd(fargs(out_moments=None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(dbuf[G:G + N].view(H, W), dist) and torch.isnan(mbuf[G:G + 4 * N]).all()
    assert _counters() == (before[0] + 3, before[1])   # (forward_map's call among them)
    fresh()
    assert fwd(fargs(R=0)) == 0   # no lists to walk: zeros, no launch
    torch.cuda.synchronize()
    assert guards_ok() and not dbuf[G:G + N].any() and not mbuf[G:G + 4 * N].any() and _counters() == (before[0] + 3, before[1])

    def bargs(struct_size=C.sizeof(_BackwardArgs), options=None, **kw):
        a = _BackwardArgs()
        a.struct_size = struct_size
        a.P, a.R, a.width, a.height = P, int(frame[0]), W, H
        a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, rs.tanfovx, rs.tanfovy, rs.kernel_size
        a.background, a.subpixel_offset, a.dL_dpix = rs.bg.data_ptr(), rs.subpixel_offset.data_ptr(), dL.data_ptr()
        a.means3D, a.colors_precomp, a.scales, a.rotations = (t[k].data_ptr() for k in ("means3D", "colors_precomp", "scales", "rotations"))
        a.viewmatrix, a.projmatrix, a.campos, a.radii = rs.viewmatrix.data_ptr(), rs.projmatrix.data_ptr(), rs.campos.data_ptr(), radii.data_ptr()
        a.geom_buffer, a.binning_buffer, a.image_buffer = frame[3].data_ptr(), frame[4].data_ptr(), frame[5].data_ptr()
        a.dL_dmean2D, a.dL_dopacity, a.dL_dcolor, a.dL_dmean3D, a.dL_dscale, a.dL_drot = (outs[k].data_ptr() for k in ("mean2D", "opacity", "color", "mean3D", "scale", "rot"))
        a.stream = stream
        if options is not None:
            a.options = C.pointer(options)
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def block(**kw):
        b = _DistortionGrad(C.sizeof(_DistortionGrad), dLt.data_ptr(), mom.data_ptr(), v.data_ptr(), vbuf[G:].data_ptr())
        for k, val in kw.items():
            setattr(b, k, val)
        return b

    def call(a, b=None, extras_size=C.sizeof(_BackwardExtras), null_extras=False):
        if null_extras:
            return lib.wg_rasterize_backward_with(C.byref(a), None)
        ex = _BackwardExtras(extras_size, C.pointer(b) if b is not None else None)
        return lib.wg_rasterize_backward_with(C.byref(a), C.byref(ex))
    fresh()
    refused = [(bargs(), block(struct_size=32)), (bargs(), block(dL_ddistortion=None)), (bargs(), block(moments=None)), (bargs(), block(dL_dvalues=None)),
               (bargs(campos=None), block(values=None)), (bargs(means3D=None), block(values=None)),
               (bargs(options=_CallOptions(1, 1, 1)), block()), (bargs(options=_CallOptions(1, 0, 0)), block()),
               (bargs(colour_gradients_only=1), block()), (bargs(colour_gradients_only=2), block())]
    for i, (a, b) in enumerate(refused):
        assert call(a, b) == -1, i
    assert call(bargs(), block(), extras_size=8) == -1   # a short extras struct
    torch.cuda.synchronize()
    assert torch.isnan(vbuf[G:G + P]).all() and all(torch.isnan(o).all() for o in outs.values()) and _counters()[1] == before[1]
    # NULL extras and a NULL block: wg_rasterize_backward_ex
    assert lib.wg_rasterize_backward_ex(C.byref(bargs())) == 0
    torch.cuda.synchronize()
    without = {k: o.clone() for k, o in outs.items()}
    for kw in (dict(null_extras=True), dict()):
        fresh()
        assert call(bargs(), None, **kw) == 0
        torch.cuda.synchronize()
        assert torch.isnan(vbuf[G:G + P]).all() and _counters()[1] == before[1]
        for k in outs:
            assert rel_err(outs[k].cpu().numpy(), without[k].cpu().numpy()) <= ORDER_BAR, k
    want = _operator_sum("ragged", "values", True)
    for values in (v.data_ptr(), None):
        fresh()
        assert call(bargs(), block(values=values)) == 0
        torch.cuda.synchronize()
        assert guards_ok() and torch.isfinite(vbuf).all()
        assert rel_err(vbuf[G:G + P].double().cpu().numpy(), want["values"]) <= GRAD_BAR
        assert rel_err(outs["color"].cpu().numpy(), without["color"].cpu().numpy()) <= ORDER_BAR   # record slots 0..2 are the image's alone
        assert rel_err(outs["mean2D"].double().cpu().numpy(), want["means2D"]) <= GRAD_BAR
    assert _counters()[1] == before[1] + 2
    fresh()
    assert call(bargs(R=0), block()) == 0   # R = 0: dL_dvalues zero-filled, no walk
    torch.cuda.synchronize()
    assert not vbuf[G:G + P].any() and guards_ok() and _counters()[1] == before[1] + 2
    assert lib.wg_set_option(b"distortion_calls", 1) != 0 and lib.wg_set_option(b"distortion_grad_calls", 1) != 0   # read-only


# ---- 12. captured replay --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_calls_replay_the_eager_results():
    from diff_gaussian_rasterization import _C
    sc = L.scene("ragged")
    P = sc["cloud"]["means3D"].shape[0]
    rs = L.settings(sc)
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    dL, dLt = to_dev(sc["cot"]), to_dev(sc["cot_t"])
    frame = _native_frame(_C, rs, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up on the capture stream; the first backward call also consumes the frame's clean-record mark
            dist, mom = _native_distortion(_C, rs, P, frame, "distance", t, moments=True)
            want = _native_backward(_C, rs, t, frame, dL, distortion=(dLt, mom, "distance"))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dist_g, mom_g = _native_distortion(_C, rs, P, frame, "distance", t, moments=True)
        got = _native_backward(_C, rs, t, frame, dL, distortion=(dLt, mom_g, "distance"))
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dist_g, dist) and torch.equal(mom_g, mom)   # the forward pass replays the eager bits
    for k, a, b in zip(NATIVE_NAMES + ("values",), got, want):
        if a is not None and a.numel():
            assert torch.isfinite(a).all(), k
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= ORDER_BAR, k
    assert float(got[8].abs().max()) > 0


@pytest.mark.gpu
def test_under_no_grad_on_a_reused_frame_and_beside_contributions(options):
    from diff_gaussian_rasterization import ContributionStats, GaussianRasterizer, _C
    sc = L.scene("ragged")
    P = sc["cloud"]["means3D"].shape[0]
    base = L.forward_map(sc, "distance")
    rs = L.settings(sc)
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    kw = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    stats = ContributionStats(P, "cuda")
    with torch.no_grad():
        out = GaussianRasterizer(rs)(**kw, colors_precomp=t["colors_precomp"], return_distortion="distance", contributions=stats)
    assert len(out) == 4 and torch.equal(out[-1], base) and stats.views == 1 and int(stats.hits.sum()) > 0
    options(geometry_reuse=1)
    hits = _C.geometry_reuse_hits()
    with torch.no_grad():
        GaussianRasterizer(rs)(**kw, colors_precomp=t["colors_precomp"])
        out = GaussianRasterizer(rs)(**kw, colors_precomp=1.0 - t["colors_precomp"], return_distortion="distance")
    assert _C.geometry_reuse_hits() == hits + 1 and torch.equal(out[-1], base)


# ---- 13. what needs no device ---------------------------------------------------------------------------------------------------------------
def _cpu_call(**fwd):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    P = 5
    rs = GaussianRasterizationSettings(image_height=4, image_width=6, tanfovx=1.0, tanfovy=1.0, kernel_size=0.1, subpixel_offset=torch.zeros(4, 6, 2),
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False, return_accumulation=False)
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), colors_precomp=torch.ones(P, 3),
              scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    kw.update(fwd)
    return GaussianRasterizer(rs)(**kw)


def test_keyword_validation_without_a_device():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import _C
    for fn in (D.rasterize_gaussians, D.GaussianRasterizer.forward):
        p = inspect.signature(fn).parameters
        assert p["return_distortion"].kind is inspect.Parameter.KEYWORD_ONLY and p["return_distortion"].default is None
        assert p["distortion_grad"].kind is inspect.Parameter.KEYWORD_ONLY and p["distortion_grad"].default is False
    assert not _C.distortion_grad_refused(False, (1, 0, 1)) and not _C.distortion_grad_refused(False, (0, 0, 1), False)
    for bad in ((True, (1, 0, 1)), ("fixed_order", (1, 0, 1)), (False, (1, 1, 1)), (False, (1, 0, 0)), (False, (1, 0, 1), True)):
        assert _C.distortion_grad_refused(*bad), bad
    for source in ("distance", torch.zeros(5)):
        for kw in (dict(colour_gradients_only=True), dict(colour_gradients_only="fixed_order"), dict(deterministic_backward=True), dict(grad_record=False),
                   dict(binning_capacity=100)):
            with pytest.raises(Exception) as info:   # refused at forward time, before anything is rendered
                _cpu_call(return_distortion=source, distortion_grad=True, **kw)
            assert str(info.value) == _C.DISTORTION_GRAD_MSG, kw
        with pytest.raises(Exception) as info:
            _cpu_call(return_distortion=source, binning_capacity=100)
        assert str(info.value) == _C.DISTORTION_CAPACITY_MSG
    with pytest.raises(Exception, match="pass return_distortion too"):
        _cpu_call(distortion_grad=True)
    for bad in ("nearest", ""):
        with pytest.raises(ValueError, match="return_distortion must be"):   # an unknown string: before any device work
            _cpu_call(return_distortion=bad)
        with pytest.raises(ValueError, match="return_distortion must be"):
            _C.check_distortion_source(bad)
    for bad in (3.0, torch.zeros(5, dtype=torch.float64), [1.0]):
        with pytest.raises(RuntimeError, match="return_distortion must be"):
            _cpu_call(return_distortion=bad)
    with pytest.raises(RuntimeError, match="P elements"):
        _cpu_call(return_distortion=torch.zeros(4))
    cot, mom = torch.zeros(3, 4, 6), torch.zeros(4, 4, 6)
    for block, msg in (((torch.zeros(4, 6), mom), _C.DISTORTION_GRAD_BLOCK_MSG), ("distance", _C.DISTORTION_GRAD_BLOCK_MSG),
                       ((torch.zeros(4, 5), mom, "distance"), _C.DISTORTION_GRAD_COTANGENT_MSG), ((None, mom, "distance"), _C.DISTORTION_GRAD_COTANGENT_MSG),
                       ((torch.zeros(4, 6), mom[:3], "distance"), _C.DISTORTION_GRAD_MOMENTS_MSG), ((torch.zeros(4, 6), None, "distance"), _C.DISTORTION_GRAD_MOMENTS_MSG),
                       ((torch.zeros(4, 6), mom, torch.zeros(4)), "distortion values must have P elements")):
        with pytest.raises(RuntimeError) as info:
            _C._check_distortion_grad_arguments(block, 5, cot)
        assert str(info.value) == msg, block
    _C._check_distortion_grad_arguments((torch.zeros(4, 6), mom, "distance"), 5, cot)


def test_output_and_cotangent_arity_without_a_device(monkeypatch):
    """The native module is replaced by stand-ins: only the tuple logic of the autograd function runs."""
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import _C
    calls, walks = [], []

    def fake_forward(*a, colors2=None, **kw):
        e = torch.empty(0, dtype=torch.uint8)
        return (7, torch.zeros(3, 4, 6), torch.zeros(5, dtype=torch.int32), e, e, e) + ((torch.ones(3, 4, 6),) if colors2 is not None else ())

    def fake_depth(geom, binning, img, R, P, H, W, source, *a, **kw):
        return torch.full((H, W), 2.0)

    def fake_distortion(geom, binning, img, R, P, H, W, source, *a, moments=False, **kw):
        walks.append(moments)
        d = torch.full((H, W), 5.0)
        return (d, torch.full((4, H, W), 6.0)) if moments else d

    def fake_backward(*a, depth=None, distortion=None, dL_dout_color2=None, **kw):
        dL = a[14]
        calls.append(dict(depth=depth, distortion=distortion, dL=dL.clone(), second=dL_dout_color2 is not None))
        P = 5
        out = (torch.ones(P, 3), torch.ones(P, 3), torch.ones(P, 1), torch.ones(P, 3), None, torch.zeros(P, 0, 3), torch.ones(P, 3), torch.ones(P, 4))
        if dL_dout_color2 is not None:
            out += (torch.ones(P, 3),)
        return out + ((torch.full((P,), 4.0),) if distortion is not None else ()) + ((torch.full((P,), 3.0),) if depth is not None else ())
    monkeypatch.setattr(_C, "rasterize_gaussians", fake_forward)
    monkeypatch.setattr(_C, "render_depth", fake_depth)
    monkeypatch.setattr(_C, "render_distortion", fake_distortion)
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", fake_backward)
    fwd = list(inspect.signature(D._RasterizeGaussians.forward).parameters)
    assert fwd[-4:] == ["distortion_grad", "return_distortion", "depth_grad", "return_depth"]

    def leaves():
        return dict(means3D=torch.zeros(5, 3, requires_grad=True), opacities=torch.ones(5, 1, requires_grad=True))
    assert len(_cpu_call()) == 3 and not walks
    # False / absent: one more output that takes no gradient, no moments kept
    for kw in (dict(), dict(distortion_grad=False)):
        out = _cpu_call(return_distortion="distance", **leaves(), **kw)
        assert len(out) == 4 and out[0].requires_grad and not out[-1].requires_grad and float(out[-1][0, 0]) == 5.0
    assert walks == [False, False]
    # True, distance: the cotangent arrives with the moments and the source; a loss on the map alone runs on a zero image cotangent
    t = leaves()
    out = _cpu_call(return_distortion="distance", distortion_grad=True, **t)
    assert len(out) == 4 and out[-1].requires_grad and walks[-1] is True
    (out[-1] * 0.5).sum().backward()
    blk = calls[0]["distortion"]
    assert len(calls) == 1 and blk[2] == "distance" and torch.equal(blk[0], torch.full((4, 6), 0.5)) and torch.equal(blk[1], torch.full((4, 4, 6), 6.0))
    assert not calls[0]["dL"].any() and calls[0]["dL"].shape == (3, 4, 6) and calls[0]["depth"] is None
    assert torch.equal(t["means3D"].grad, torch.ones(5, 3))
    # a tensor that requires grad takes the distortion's dL_dvalues
    t, values = leaves(), torch.zeros(5, requires_grad=True)
    out = _cpu_call(return_distortion=values, distortion_grad=True, **t)
    (out[0].sum() + out[-1].sum()).backward()
    assert len(calls) == 2 and not calls[1]["distortion"][2].requires_grad and torch.equal(values.grad, torch.full((5,), 4.0))
    # a None cotangent sends no block
    t = leaves()
    out = _cpu_call(return_distortion="distance", distortion_grad=True, **t)
    out[0].sum().backward()
    assert len(calls) == 3 and calls[2]["distortion"] is None
    # beside depth and a second image: (color, radii, accumulation, color2, depth, distortion); each tensor takes its own gradient
    t, vd, vt = leaves(), torch.zeros(5, requires_grad=True), torch.zeros(5, requires_grad=True)
    out = _cpu_call(return_depth=vd, depth_grad=True, return_distortion=vt, distortion_grad=True, colors_precomp2=torch.ones(5, 3), **t)
    assert len(out) == 6 and float(out[4].detach()[0, 0]) == 2.0 and float(out[5].detach()[0, 0]) == 5.0
    (out[4].sum() * 2 + out[5].sum() * 3).backward()
    c = calls[3]
    assert c["second"] and torch.equal(c["depth"][0], torch.full((4, 6), 2.0)) and torch.equal(c["distortion"][0], torch.full((4, 6), 3.0))
    assert torch.equal(vd.grad, torch.full((5,), 3.0)) and torch.equal(vt.grad, torch.full((5,), 4.0))
    # one tensor feeding both takes the sum; depth alone beside an unused map sends depth's block only
    t, both = leaves(), torch.zeros(5, requires_grad=True)
    out = _cpu_call(return_depth=both, depth_grad=True, return_distortion=both, distortion_grad=True, **t)
    assert len(out) == 5
    (out[3].sum() + out[4].sum()).backward()
    assert torch.equal(both.grad, torch.full((5,), 7.0))
    t = leaves()
    out = _cpu_call(return_depth="distance", depth_grad=True, return_distortion="distance", distortion_grad=True, **t)
    out[3].sum().backward()
    assert calls[-1]["depth"] is not None and calls[-1]["distortion"] is None
