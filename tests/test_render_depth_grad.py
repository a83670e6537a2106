"""The gradient of the depth pass (wg_depth_grad; csrc/depth/depth_bwd.hip: render_depth_backward_kernel): `GaussianRasterizer.forward(...,
return_depth=, depth_grad=True)` makes `depth` differentiable -- one more per-tile walk in the frame's backward call, adding into the gradient
record the image walk fills.

The yardstick throughout is the operator's own existing path, TWO CALLS: (i) the same call without depth under the image cotangent, (ii) a
three-channel call with colors_precomp = v[:, None].repeat(1, 3), an all-zero background and the cotangent (dL_ddepth, 0, 0); their gradients
added (in float64), colors_precomp.grad[:, 0] of (ii) as dL/dv, and in distance mode the direct term dL/dv (x - campos) / v added in float64.

Bars: 1e-3 max-rel-err against the float32 oracle's two calls (the project's gradient bar); against the float64 oracle's two calls at most
twice the operator's own two calls' error (tests/test_colour_backward.py's rule); the identity sum_g dL/dv_g v_g = <dL_ddepth, depth> at most
twice the three-channel call's residual on <colors.grad, colors> = <cot, image>; 2e-6 of an array's largest magnitude between two orders of
the same float32 sums (ORDER_BAR, docs/OPTIONS.md)."""
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
    "saturating": (1500, 320, 200, 12.0, False),  # long lists, pixels that stop early through n_contrib
    "plain": (10000, 256, 256, 1.0, False),
}
BG = (0.2, 0.5, 0.8)
ORDER_BAR = 2e-6   # two orders of the same float32 sums (tests/test_colour_backward.py, docs/OPTIONS.md)
GRAD_BAR = 1e-3    # the project's gradient bar
GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations")

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _make_scene(name):
    """-> dict(cloud: numpy arrays, cam, so: sub-pixel offsets or None, cot: image cotangent [3,H,W], cot_d: depth cotangent [H,W],
    v: the float32 distances to the camera, as torch computes them)"""
    if name == "dense":   # ~1000 instances per tile (tests/test_colour_backward.py: _dense): lists the lazy sort engages on at test thresholds
        P, W, H, sm, offsets, seed = 30000, 320, 200, 7.0, False, 5
    else:
        (P, W, H, sm, offsets), seed = SCENES[name], 11
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=seed, scale_mult=sm)
    cam = S.make_camera(W, H)
    so = np.random.default_rng(3).uniform(-0.5, 0.5, size=(H, W, 2)).astype(np.float32) if offsets else None
    return _with_cotangents(cloud, cam, so)


def _with_cotangents(cloud, cam, so=None):
    W, H = cam["width"], cam["height"]
    v = torch.norm(torch.from_numpy(cloud["means3D"]) - torch.from_numpy(np.asarray(cam["campos"], np.float32))[None], dim=-1).numpy()
    return dict(cloud=cloud, cam=cam, so=so, cot=S.make_cotangent(W, H), cot_d=np.ascontiguousarray(3.0 * S.make_cotangent(W, H, seed=7)[0]), v=v)


def _scene(name):
    return _cached(("scene", name), lambda: _make_scene(name))


def _leaves(sc):
    t = {k: to_dev(v).requires_grad_(True) for k, v in sc["cloud"].items()}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    return t


def _geo(t):
    return dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])


def _grads(t, **more):
    g = {k: None if t[k].grad is None else t[k].grad.detach().cpu().numpy().astype(np.float64) for k in GEOMETRY + ("colors_precomp",) if k in t}
    g.update(more)
    return g


def _new(sc, mode, image=True, exact=True, bg=BG, **fwd):
    """One call with return_depth= and depth_grad=True, a loss on depth (and on the image) -> dict(grads, depth, color)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(sc["cam"], 0, bg=np.array(bg, np.float32), subpixel_offset=sc["so"])
    t = _leaves(sc)
    values = to_dev(sc["v"]).requires_grad_(True) if mode == "values" else None
    out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], return_depth="distance" if values is None else values, depth_grad=True,
                                 exact_compositing=bool(exact), **fwd)
    depth = out[-1]
    assert depth.requires_grad
    loss = (depth * to_dev(sc["cot_d"])).sum()
    if image:
        loss = loss + (out[0] * to_dev(sc["cot"])).sum()
    loss.backward()
    return dict(grads=_grads(t, values=None if values is None else values.grad.detach().cpu().numpy().astype(np.float64)),
                depth=depth.detach().cpu().numpy(), color=out[0].detach().cpu().numpy())


def _direct_term(sc, dv):
    """dL/dv (x - campos) / v in float64, 0 where v == 0"""
    d = sc["cloud"]["means3D"].astype(np.float64) - np.asarray(sc["cam"]["campos"], np.float64)[None]
    v = np.linalg.norm(d, axis=1)
    return np.where(v[:, None] > 0, dv[:, None] * d / np.where(v > 0, v, 1.0)[:, None], 0.0)


def _sum_two(sc, one, two, mode, image):
    """Two calls' gradients added in float64: `one` = (i) or None, `two` = (ii) with dL/dv under "values"."""
    out = {}
    for k in GEOMETRY:
        out[k] = np.asarray(two[k], np.float64) + (np.asarray(one[k], np.float64) if image else 0.0)
    out["values"] = np.asarray(two["values"], np.float64)
    if mode == "distance":
        out["means3D"] = out["means3D"] + _direct_term(sc, out["values"])
    return out


def _operator_call_one(sc, exact=True):
    """(i): the same call without depth under the image cotangent"""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32), subpixel_offset=sc["so"])
    t = _leaves(sc)
    out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], exact_compositing=bool(exact))
    out[0].backward(to_dev(sc["cot"]))
    return _grads(t)


def _operator_call_two(sc, exact=True, **fwd):
    """(ii): the three-channel call with the scalars as colours over a zero background under (dL_ddepth, 0, 0) -> gradients, dL/dv, and the
    residual of its own identity <colors.grad, colors> = <cot, image>"""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(sc["cam"], 0, subpixel_offset=sc["so"])
    t = _leaves(sc)
    colors = to_dev(sc["v"])[:, None].repeat(1, 3).requires_grad_(True)
    cot3 = torch.zeros(3, sc["cam"]["height"], sc["cam"]["width"], device="cuda")
    cot3[0] = to_dev(sc["cot_d"])
    out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=colors, exact_compositing=bool(exact), **fwd)
    out[0].backward(cot3)
    g = _grads(t, values=colors.grad[:, 0].detach().cpu().numpy().astype(np.float64))
    lhs = float((colors.grad.double() * colors.detach().double()).sum())
    rhs = float((cot3.double() * out[0].detach().double()).sum())
    g["identity_residual"] = abs(lhs - rhs) / abs(rhs)
    return g


def _operator_two_calls(name, mode, image, exact=True):
    sc = _scene(name)
    one = _cached(("op-i", name, exact), lambda: _operator_call_one(sc, exact)) if image else None
    two = _cached(("op-ii", name, exact), lambda: _operator_call_two(sc, exact))
    return _sum_two(sc, one, two, mode, image)


def _oracle_two_calls(oracle, name, mode, image, precision):
    sc = _scene(name)

    def run(which):
        if which == "i":
            o = oracle.run_scene(sc["cloud"], sc["cam"], sh_degree=0, cotangent=sc["cot"], bg=np.array(BG, np.float32), subpixel_offset=sc["so"],
                                 precision=precision)
        else:
            cot3 = np.zeros_like(sc["cot"])
            cot3[0] = sc["cot_d"]
            cloud = dict(sc["cloud"], colors_precomp=np.ascontiguousarray(np.repeat(sc["v"][:, None], 3, axis=1)))
            o = oracle.run_scene(cloud, sc["cam"], sh_degree=0, cotangent=cot3, subpixel_offset=sc["so"], precision=precision)
        g = {k: np.asarray(o["grads"][k], np.float64).reshape(sc["cloud"]["means3D"].shape[0], -1) for k in GEOMETRY}
        g["values"] = np.asarray(o["grads"]["colors_precomp"], np.float64).reshape(-1, 3)[:, 0]
        return g
    one = _cached(("oracle-i", name, precision), lambda: run("i")) if image else None
    two = _cached(("oracle-ii", name, precision), lambda: run("ii"))
    return _sum_two(sc, one, two, mode, image)


def _errors(got, ref, mode):
    """name -> rel_err over the gradients the issue lists (values: values mode only; in distance mode dL/dv reaches means3D)"""
    names = GEOMETRY + (("values",) if mode == "values" else ())
    return {k: rel_err(np.asarray(got[k]).reshape(np.asarray(ref[k]).shape), ref[k]) for k in names}


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


def _counter():
    from diff_gaussian_rasterization import _C
    return _C.get_option("depth_grad_calls")


# ---- 1. against the float32 oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("image", [True, False], ids=["image+depth", "depth-only"])
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("mode", ["values", "distance"])
@pytest.mark.parametrize("exact", [1, 0])
def test_gradients_match_the_float32_oracles_two_calls(oracle, exact, mode, name, image):
    sc = _scene(name)
    before = _counter()
    got = _new(sc, mode, image, exact)
    assert _counter() == before + 1
    ref = _oracle_two_calls(oracle, name, mode, image, "f32")
    errs = _errors(got["grads"], ref, mode)
    print(f"{name} / {mode} / exact={exact} / image={image}: rel_err against the float32 oracle's two calls: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    for k in GEOMETRY:
        assert np.abs(ref[k]).max() > 0, k
    assert np.abs(ref["means2D"][:, 2]).max() > 0   # the abs term: held to "as two calls accumulate"
    for k, e in errs.items():
        assert e <= GRAD_BAR, (k, e)
    # the abs term on its own scale (x and y are NDC-scaled and far larger)
    assert rel_err(got["grads"]["means2D"][:, 2], ref["means2D"][:, 2]) <= GRAD_BAR
    if mode == "distance":
        assert got["grads"]["values"] is None


# ---- 2. against the float64 oracle, relative to the existing pass ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("image", [True, False], ids=["image+depth", "depth-only"])
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("mode", ["values", "distance"])
def test_error_against_float64_is_at_most_twice_the_two_calls(oracle, mode, name, image):
    """Per gradient: rel_err of the new path against the float64 oracle's two calls <= 2 x that of the operator's own two calls (the rule and
    the factor of tests/test_colour_backward.py: test_error_against_float64_is_at_most_twice_the_full_backward_passes -- one more independent
    float32 evaluation)."""
    sc = _scene(name)
    ref = _oracle_two_calls(oracle, name, mode, image, "f64")
    e_new = _errors(_cached(("new", name, mode, image, 1), lambda: _new(sc, mode, image, 1))["grads"], ref, mode)
    e_two = _errors(_operator_two_calls(name, mode, image), ref, mode)
    print(f"{name} / {mode} / image={image}: rel_err against the float64 oracle, new path | two calls: " +
          ", ".join(f"{k} {e_new[k]:.3e} | {e_two[k]:.3e}" for k in e_new))
    if os.environ.get("WG_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "render_depth", "accuracy_grad.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[f"{name}/{mode}/{'image+depth' if image else 'depth-only'}"] = {k: dict(rel_err_f64_new_path=e_new[k], rel_err_f64_two_calls=e_two[k]) for k in e_new}
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    for k in e_new:
        assert e_new[k] <= GRAD_BAR, (k, e_new[k])
        if e_two[k] > 0:
            assert e_new[k] <= 2 * e_two[k], (k, e_new[k], e_two[k])


# ---- 3. tied to the forward depth -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_value_gradients_reproduce_the_forward_depth(name):
    """depth is linear in v: sum_g dL/dv_g v_g = <dL_ddepth, depth>.  The relative residual (inner products in float64) is at most twice that
    of the three-channel call (ii) on its own identity <colors.grad, colors> = <cot, image>."""
    sc = _scene(name)
    new = _cached(("new", name, "values", False, 1), lambda: _new(sc, "values", False, 1))
    lhs = float((new["grads"]["values"] * sc["v"].astype(np.float64)).sum())
    rhs = float((sc["cot_d"].astype(np.float64) * new["depth"].astype(np.float64)).sum())
    res_new = abs(lhs - rhs) / abs(rhs)
    res_two = _cached(("op-ii", name, True), lambda: _operator_call_two(sc, True))["identity_residual"]
    print(f"{name}: identity residual, new path {res_new:.3e}, three-channel call {res_two:.3e}")
    assert abs(rhs) > 0
    assert res_new <= 2 * res_two


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------------
def _one_tile(P):
    """tests/test_render_depth.py: _one_tile -- one 16 x 16 tile, P faint Gaussians that all cover it: the walk's batches end where the list does."""
    rng = np.random.default_rng(P)
    z = rng.uniform(2.0, 8.0, size=P)
    means = np.stack([0.02 * z * rng.uniform(-1, 1, size=P), 0.02 * z * rng.uniform(-1, 1, size=P), z], axis=1)
    scales = (1.5 * z)[:, None] * np.ones((P, 3))
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    cloud = dict(means3D=means, scales=scales, rotations=q, opacities=np.full((P, 1), 0.01), colors_precomp=rng.uniform(0, 1, size=(P, 3)))
    return _with_cotangents({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in cloud.items()}, S.make_camera(16, 16))


def _against_two_calls(sc, mode, image=True, exact=True, **fwd):
    """the new path against the operator's own two calls on a scene outside the cache -> the errors"""
    got = _new(sc, mode, image, exact, **fwd)
    ref = _sum_two(sc, _operator_call_one(sc, exact) if image else None, _operator_call_two(sc, exact), mode, image)
    return _errors(got["grads"], ref, mode), got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 200])
def test_batch_edges_on_one_tile(P, exact):
    sc = _one_tile(P)
    for mode in ("values", "distance"):
        errs, got, ref = _against_two_calls(sc, mode, True, exact)
        print(f"one tile, P = {P}, exact={exact}, {mode}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
        assert np.abs(ref["values"]).min() > 0   # the premise: every Gaussian is blended
        for k, e in errs.items():
            if k != "rotations":
                assert e <= GRAD_BAR, (mode, k, e)
        # rotations: these Gaussians are isotropic (three equal scales), so their rotation gradient is ZERO in exact arithmetic and both sides hold
        # only the rounding of the terms that cancel -- dL/dM dM/dq with M = S R, each of the size of |dL/dscale| * scale.  The difference is held
        # to the bar on that scale; a ratio of the two noises says nothing.
        scale = np.abs(ref["scales"]).max() * float(sc["cloud"]["scales"].max())
        d_rot = np.abs(got["grads"]["rotations"] - ref["rotations"]).max()
        print(f"    rotations (zero in exact arithmetic): largest difference {d_rot:.3e} on the scale {scale:.3e}")
        assert d_rot <= GRAD_BAR * scale, (mode, d_rot, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (17, 33)])
def test_small_and_ragged_images(size):
    W, H = size
    sc = _with_cotangents(S.make_cloud(400, W, H, sh_degree=None, seed=2, scale_mult=20.0), S.make_camera(W, H))
    for mode in ("values", "distance"):
        errs, got, ref = _against_two_calls(sc, mode)
        assert np.abs(ref["values"]).max() > 0
        for k, e in errs.items():
            assert e <= GRAD_BAR, (mode, k, e)


@pytest.mark.gpu
def test_empty_frames_leave_zero_gradients_and_the_counter_alone():
    """P = 0; everything culled, which is R = 0: zero gradients, no walk."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = _scene("ragged")
    before = _counter()
    behind = dict(sc, cloud=dict(sc["cloud"], means3D=sc["cloud"]["means3D"] * np.array([1, 1, -1], np.float32)))
    for mode in ("values", "distance"):
        got = _new(behind, mode)
        assert not got["depth"].any()
        for k in GEOMETRY + (("values",) if mode == "values" else ()):
            assert got["grads"][k] is not None and not got["grads"][k].any(), (mode, k)
    rs = make_settings(sc["cam"], 0)
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    for source in ("distance", z(0)):
        t = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
        out = GaussianRasterizer(rs)(**t, return_depth=source, depth_grad=True)
        (out[-1].sum() + out[0].sum()).backward()
        assert t["means3D"].grad is not None and t["means3D"].grad.shape == (0, 3)
        if isinstance(source, torch.Tensor):
            assert source.grad is not None and source.grad.shape == (0,)
    assert _counter() == before


@pytest.mark.gpu
def test_pixels_without_a_contributor_beside_pixels_that_stopped_early():
    """the Gaussians of "saturating" that lie to the right of the image's middle (tests/test_render_depth.py)"""
    sc = _scene("saturating")
    keep = sc["cloud"]["means3D"][:, 0] > 0.15 * sc["cloud"]["means3D"][:, 2]
    half = _with_cotangents({k: np.ascontiguousarray(v[keep]) for k, v in sc["cloud"].items()}, sc["cam"])
    errs, got, ref = _against_two_calls(half, "values")
    assert int((got["depth"] == 0).sum()) > 1000 and int((got["depth"] > 0).sum()) > 1000
    for k, e in errs.items():
        assert e <= GRAD_BAR, (k, e)


@pytest.mark.gpu
def test_a_gaussian_at_distance_zero_gets_a_finite_gradient_and_no_direct_term():
    """campos is a settings field of its own: put it ON a visible Gaussian's mean (the view matrix stays), so that v_g = 0 exactly while g is
    blended.  Distance mode then equals values mode with v = torch.norm(means3D - campos) under autograd, whose subgradient at 0 is 0."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = _scene("plain")
    dv_ref = _cached(("op-ii", "plain", True), lambda: _operator_call_two(sc, True))["values"]
    g = int(np.argmax(np.abs(dv_ref)))   # a Gaussian that certainly takes a depth gradient
    cam = dict(sc["cam"], campos=sc["cloud"]["means3D"][g].copy())
    rs = make_settings(cam, 0, bg=np.array(BG, np.float32))
    cot_d = to_dev(sc["cot_d"])
    grads = {}
    for mode in ("distance", "values"):
        t = _leaves(sc)
        source = "distance" if mode == "distance" else torch.norm(t["means3D"] - rs.campos[None], dim=-1)
        if mode == "values":
            assert float(source[g]) == 0.0
        out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], return_depth=source, depth_grad=True)
        (out[-1] * cot_d).sum().backward()
        grads[mode] = _grads(t)
    for k in GEOMETRY:
        assert np.isfinite(grads["distance"][k]).all(), k
        assert rel_err(grads["distance"][k], grads["values"][k]) <= GRAD_BAR, k
    # g itself: what is left at v = 0 is the chain through the record alone
    scale = np.abs(grads["values"]["means3D"]).max()
    assert np.abs(grads["distance"]["means3D"][g] - grads["values"]["means3D"][g]).max() <= GRAD_BAR * scale


@pytest.mark.gpu
def test_a_nan_value_stays_with_the_gaussians_it_shares_a_pixel_with():
    """No claim beyond that: a Gaussian whose tile rectangle is disjoint from the NaN Gaussian's shares no pixel with it."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    from wg_testlib import run_hip_native
    sc = _scene("plain")
    n = run_hip_native(sc["cloud"], sc["cam"], sh_degree=0)
    sp = n["views"]["geometry"]["splats"].cpu().numpy()
    radii = n["radii"].cpu().numpy()
    mx, my = sp[:, 0], sp[:, 1]
    inside = (radii > 0) & (mx > 100) & (mx < 156) & (my > 100) & (my < 156)
    g = int(np.flatnonzero(inside)[0])
    # tile rectangles are disjoint when the footprints are more than a tile apart on one axis
    far = (radii > 0) & ((np.abs(mx - mx[g]) > radii + radii[g] + 32) | (np.abs(my - my[g]) > radii + radii[g] + 32))
    assert int(far.sum()) > 1000
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32))
    t = _leaves(sc)
    values = to_dev(sc["v"]).clone()
    values[g] = float("nan")
    values.requires_grad_(True)
    out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], return_depth=values, depth_grad=True)
    ((out[-1].nan_to_num() * to_dev(sc["cot_d"])).sum() + (out[0] * to_dev(sc["cot"])).sum()).backward()
    far_t = torch.from_numpy(far).cuda()
    for k in GEOMETRY:
        assert torch.isfinite(t[k].grad[far_t]).all(), k
    assert torch.isfinite(values.grad[far_t]).all()
    assert _C.get_option("depth_grad_calls") > 0


# ---- 5. binning paths -----------------------------------------------------------------------------------------------------------------------
PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["saturating", "dense"])
def test_every_binning_path_gives_the_same_gradients(options, name, path):
    """The walk reads each tile's list up to tile_last only: behind it lie the unsorted tails of lazily sorted lists."""
    sc = _scene(name)
    base = _cached(("path-default", name), lambda: _new(sc, "distance"))   # (the library's defaults: the fixture puts them back after every test)
    options(**PATHS[path])
    got = _new(sc, "distance")
    assert np.array_equal(got["depth"], base["depth"])
    for k in GEOMETRY:
        e = rel_err(got["grads"][k], base["grads"][k])
        print(f"{name} / {path}: {k} rel_err against the default path = {e:.3e}")
        assert e <= ORDER_BAR, (k, e)
    if name == "dense":
        from wg_testlib import run_hip_native
        rg = run_hip_native(sc["cloud"], sc["cam"], sh_degree=0)["views"]["image"]["ranges"].cpu().numpy().astype(np.int64)
        assert (rg[:, 1] - rg[:, 0]).max() > 600


# ---- 6. colour sources ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_colour_source_of_the_call():
    """SH colours with forward_only = 0 (the backward-row kernel), precomputed colours, sh_second + tone2 (the thirteen-sum record), a tone, raw
    parameters: the geometry gradients are two calls' at the 1e-3 bar, and what belongs to the colours (slots 0..2, 10, 11 and grad_aux of the
    record) comes out as without depth."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    P, W, H = 3000, 160, 96
    cam = S.make_camera(W, H)
    sc = _with_cotangents(S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=3.0), cam)
    shs0 = S.make_cloud(P, W, H, sh_degree=1, seed=3, scale_mult=3.0)["shs"]
    rs = make_settings(cam, 1, bg=np.array(BG, np.float32))
    rs0 = make_settings(cam, 1)
    cot, cot_d, v = to_dev(sc["cot"]), to_dev(sc["cot_d"]), to_dev(sc["v"])
    cot3 = torch.zeros_like(cot)
    cot3[0] = cot_d
    ones = torch.ones(P, 3, device="cuda")
    f3d = torch.full((P, 1), 0.01, device="cuda")

    def leaves(raw):
        t = _leaves(sc)
        if raw:
            t["opacities"] = torch.logit(t["opacities"].detach().clamp(0.01, 0.99)).requires_grad_(True)
            t["scales"] = torch.log(t["scales"].detach()).requires_grad_(True)
        t["shs"] = to_dev(shs0).requires_grad_(True)
        t["mul"], t["mul2"], t["offset"] = (0.5 * ones).requires_grad_(True), (0.7 * ones).requires_grad_(True), (0.1 * ones).requires_grad_(True)
        return t
    sources = dict(
        shs=lambda t: dict(shs=t["shs"]),
        colors_precomp=lambda t: dict(colors_precomp=t["colors_precomp"]),
        two_tones=lambda t: dict(shs=t["shs"], sh_mul=t["mul"], sh_offset=t["offset"], sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0, sh_second=True,
                                 sh_mul2=t["mul2"], sh_pre_clamp_max2=1.0),
        tone=lambda t: dict(shs=t["shs"], sh_mul=t["mul"], sh_offset=t["offset"], sh_pre_clamp_max=1.0, sh_post_clamp_max=1.0),
        raw=lambda t: dict(colors_precomp=t["colors_precomp"], filter_3D=f3d))
    colour_leaves = ("shs", "colors_precomp", "mul", "mul2", "offset")

    def image_loss(out, two):
        return (out[0] * cot).sum() + ((out[3] * cot).sum() * 0.5 if two else 0.0)
    rows_before = _C.get_option("backward_row_calls")
    for name, make in sources.items():
        raw, two = name == "raw", name == "two_tones"
        extra = dict(filter_3D=f3d) if raw else {}
        # (i) the same call without depth
        t1 = leaves(raw)
        image_loss(GaussianRasterizer(rs)(**_geo(t1), **make(t1)), two).backward()
        # (ii) the three-channel call with the scalars as colours
        t2 = leaves(raw)
        colors = v[:, None].repeat(1, 3).requires_grad_(True)
        GaussianRasterizer(rs0)(**_geo(t2), colors_precomp=colors, **extra)[0].backward(cot3)
        # the new path
        t3 = leaves(raw)
        values = v.clone().requires_grad_(True)
        before = _counter()
        out = GaussianRasterizer(rs)(**_geo(t3), **make(t3), return_depth=values, depth_grad=True)
        (image_loss(out, two) + (out[-1] * cot_d).sum()).backward()
        assert _counter() == before + 1, name
        for k in GEOMETRY:
            ref = t1[k].grad.double() + t2[k].grad.double()
            e = rel_err(t3[k].grad.cpu().numpy(), ref.cpu().numpy())
            print(f"{name}: {k} rel_err against two calls = {e:.3e}")
            assert e <= GRAD_BAR, (name, k, e)
        assert rel_err(values.grad.cpu().numpy(), colors.grad[:, 0].cpu().numpy()) <= GRAD_BAR, name
        seen = 0
        for k in colour_leaves:   # the colours' own gradients: the call without depth (SH colours: dL_dmeans3D's direction term belongs to (i) too)
            assert (t1[k].grad is None) == (t3[k].grad is None), (name, k)
            if t1[k].grad is not None:
                seen += 1
                assert float(t1[k].grad.abs().max()) > 0, (name, k)
                assert rel_err(t3[k].grad.cpu().numpy(), t1[k].grad.cpu().numpy()) <= ORDER_BAR, (name, k)
        assert seen >= 1, name
    assert _C.get_option("backward_row_calls") > rows_before   # the SH call ran on the frame's backward rows


# ---- 7. nothing moves without it ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_loss_without_depth_is_the_call_without_the_keyword():
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = _scene("ragged")
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32), subpixel_offset=sc["so"])
    base = _cached(("op-i", "ragged", True), lambda: _operator_call_one(sc, True))
    before = _counter()
    t = _leaves(sc)
    out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], return_depth="distance", depth_grad=True)
    assert out[-1].requires_grad
    out[0].backward(to_dev(sc["cot"]))   # depth takes no cotangent: None reaches the backward call
    got = _grads(t)
    assert _counter() == before
    for k in GEOMETRY + ("colors_precomp",):
        assert rel_err(got[k], base[k]) <= ORDER_BAR, k
    # depth_grad = False (and the default): depth takes no gradient, as before
    for kw in (dict(depth_grad=False), dict()):
        t = _leaves(sc)
        out = GaussianRasterizer(rs)(**_geo(t), colors_precomp=t["colors_precomp"], return_depth="distance", **kw)
        assert out[0].requires_grad and not out[-1].requires_grad
    assert _counter() == before


# ---- 8. surface -----------------------------------------------------------------------------------------------------------------------------
def _native_frame(_C, rs, t, **fwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                  rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0, rs.campos, False, False, **fwd)


def _native_backward(_C, rs, t, frame, dL, **bwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians_backward(rs.bg, t["means3D"], frame[2], t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                           rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, dL, e, 0, rs.campos,
                                           frame[3], frame[0], frame[4], frame[5], False, **bwd)


NATIVE_NAMES = ("means2D", "colors_precomp", "opacities", "means3D", "cov3Ds_precomp", "sh", "scales", "rotations")


@pytest.mark.gpu
def test_native_call_and_refusals_under_both_bindings(binding):
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    sc = _scene("ragged")
    P, H, W = sc["cloud"]["means3D"].shape[0], 130, 250
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32), subpixel_offset=sc["so"])
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    dL, dLd, v = to_dev(sc["cot"]), to_dev(sc["cot_d"]), to_dev(sc["v"])
    want = {m: _operator_two_calls("ragged", m, True) for m in ("values", "distance")}
    geo = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
               colors_precomp=t["colors_precomp"])
    bad_block = {"not a pair": (dLd,), "cotangent size": (dLd[:-1], v), "cotangent dtype": (dLd.double(), v), "cotangent host": (dLd.cpu(), v),
                 "values size": (dLd, v[:-1]), "values dtype": (dLd, v.double()), "values host": (dLd, v.cpu()), "string": (dLd, "nearest")}
    bad_mode = {"deterministic_backward": dict(options=dict(deterministic_backward=1)), "grad_record": dict(options=dict(grad_record=0)),
                "colour_gradients_only": dict(colour_gradients_only=True), "fixed_order": dict(colour_gradients_only="fixed_order")}
    bad_operator = {"deterministic_backward": dict(deterministic_backward=True), "grad_record": dict(grad_record=False),
                    "colour_gradients_only": dict(colour_gradients_only=True), "binning_capacity": dict(binning_capacity=1_000_000)}
    said, results = {}, {}
    for name in BINDINGS:
        _C.use_binding(name)
        frame = _native_frame(_C, rs, t)
        before = _counter()
        for case, block in bad_block.items():
            with pytest.raises(RuntimeError) as info:
                _native_backward(_C, rs, t, frame, dL, depth=block)
            said[name, "block", case] = str(info.value)
        for case, kw in bad_mode.items():
            with pytest.raises(RuntimeError) as info:
                _native_backward(_C, rs, t, frame, dL, depth=(dLd, v), **kw)
            said[name, "mode", case] = str(info.value)
        for case, kw in bad_operator.items():
            for source in ("distance", v):
                with pytest.raises(Exception) as info:
                    GaussianRasterizer(rs)(**geo, return_depth=source, depth_grad=True, **kw)
                said[name, "operator", case, isinstance(source, str)] = str(info.value)
        with pytest.raises(Exception, match="pass return_depth too"):
            GaussianRasterizer(rs)(**geo, depth_grad=True)
        assert _counter() == before   # nothing was launched
        # a refused call leaves nothing behind: the well-formed ones run, eight + dL_dvalues
        for mode, source in (("values", v), ("distance", "distance")):
            res = _native_backward(_C, rs, t, frame, dL, depth=(dLd, source))
            assert len(res) == 9 and res[8].shape == (P,) and res[8].dtype == torch.float32
            got = {k: r.double().cpu().numpy().reshape(P, -1) for k, r in zip(NATIVE_NAMES, res[:8]) if k in GEOMETRY}
            got["values"] = res[8].double().cpu().numpy()
            for k in GEOMETRY + ("values",):   # (the library fills dL_dvalues in both modes)
                assert rel_err(got[k].reshape(want[mode][k].shape), want[mode][k]) <= GRAD_BAR, (name, mode, k)
            results[name, mode] = got
        assert _counter() == before + 2
        assert len(_native_backward(_C, rs, t, frame, dL)) == 8 and len(_native_backward(_C, rs, t, frame, dL, depth=None)) == 8
        assert _counter() == before + 2
    for key in [k[1:] for k in said if k[0] == "torch"]:
        assert said[("torch",) + key] == said[("ctypes",) + key], key
    assert said["torch", "block", "not a pair"] == _C.DEPTH_GRAD_BLOCK_MSG
    assert {said["torch", "block", c] for c in ("cotangent size", "cotangent dtype", "cotangent host")} == {_C.DEPTH_GRAD_COTANGENT_MSG}
    assert said["torch", "block", "values size"] == "depth values must have P elements"
    assert {said["torch", "block", c] for c in ("values dtype", "values host", "string")} == {_C.DEPTH_SOURCE_MSG}
    assert {said["torch", "mode", c] for c in bad_mode} == {_C.DEPTH_GRAD_MSG}
    assert {m for k, m in said.items() if k[0] == "torch" and k[1] == "operator"} == {_C.DEPTH_GRAD_MSG}
    for mode in ("values", "distance"):
        for k in GEOMETRY + ("values",):
            assert rel_err(results["torch", mode][k], results["ctypes", mode][k]) <= ORDER_BAR, (mode, k)


@pytest.mark.gpu
def test_c_abi_guard_words_struct_sizes_and_refusals():
    """wg_rasterize_backward_ex called directly: dL_dvalues inside a larger buffer whose guard words must survive, full of NaN on entry
    ("overwritten in full"); a wg_backward_args of the size before the block behaves as absent; every refusal is WG_ERR_INVALID_ARGUMENT and
    writes nothing."""
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _BackwardArgs, _CallOptions, _DepthGrad
    sc = _scene("ragged")
    P, H, W = sc["cloud"]["means3D"].shape[0], 130, 250
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32), subpixel_offset=sc["so"])
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    frame = _native_frame(_C, rs, t)
    dL, dLd, v = to_dev(sc["cot"]), to_dev(sc["cot_d"]), to_dev(sc["v"])
    G = 64
    buf = torch.full((G + P + G,), float("nan"), device="cuda")
    outs = {k: torch.full((P, n), float("nan"), device="cuda") for k, n in (("mean2D", 3), ("opacity", 1), ("color", 3), ("mean3D", 3), ("scale", 3), ("rot", 4))}
    radii = frame[2].contiguous()

    def fresh():
        buf.fill_(float("nan"))
        buf[:G] = 7.0
        buf[-G:] = 9.0
        for o in outs.values():
            o.fill_(float("nan"))

    def args(struct_size, block=None, options=None, **kw):
        a = _BackwardArgs()
        a.struct_size = struct_size
        a.P, a.R, a.width, a.height = P, int(frame[0]), W, H
        a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, rs.tanfovx, rs.tanfovy, rs.kernel_size
        a.background, a.subpixel_offset, a.dL_dpix = rs.bg.data_ptr(), rs.subpixel_offset.data_ptr(), dL.data_ptr()
        a.means3D, a.colors_precomp, a.scales, a.rotations = (t[k].data_ptr() for k in ("means3D", "colors_precomp", "scales", "rotations"))
        a.viewmatrix, a.projmatrix, a.campos, a.radii = rs.viewmatrix.data_ptr(), rs.projmatrix.data_ptr(), rs.campos.data_ptr(), radii.data_ptr()
        a.geom_buffer, a.binning_buffer, a.image_buffer = frame[3].data_ptr(), frame[4].data_ptr(), frame[5].data_ptr()
        a.dL_dmean2D, a.dL_dopacity, a.dL_dcolor, a.dL_dmean3D, a.dL_dscale, a.dL_drot = (outs[k].data_ptr() for k in ("mean2D", "opacity", "color", "mean3D", "scale", "rot"))
        a.stream = torch.cuda.current_stream().cuda_stream
        if options is not None:
            a.options = C.pointer(options)
        if block is not None:
            a.depth = C.pointer(block)
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def block(**kw):
        b = _DepthGrad(C.sizeof(_DepthGrad), dLd.data_ptr(), v.data_ptr(), buf[G:].data_ptr())
        for k, val in kw.items():
            setattr(b, k, val)
        return b
    full, call = C.sizeof(_BackwardArgs), lambda a: _C._lib.wg_rasterize_backward_ex(C.byref(a))
    assert full == 328 and C.sizeof(_DepthGrad) == 32
    fresh()
    before = _counter()
    refused = [args(full, block(struct_size=24)), args(full, block(dL_ddepth=None)), args(full, block(dL_dvalues=None)),
               args(full, block(values=None), campos=None), args(full, block(values=None), means3D=None),
               args(full, block(), _CallOptions(1, 1, 1)), args(full, block(), _CallOptions(1, 0, 0)), args(full, block(), colour_gradients_only=1),
               args(full, block(), colour_gradients_only=2)]
    for i, a in enumerate(refused):
        assert call(a) == -1, i
    torch.cuda.synchronize()
    assert torch.isnan(buf[G:G + P]).all() and all(torch.isnan(o).all() for o in outs.values())   # a refused call writes nothing
    assert _counter() == before
    # a struct of the size before the block: the pointer behind it is not read -- today's call
    old = args(full - 8, block())
    assert call(old) == 0
    torch.cuda.synchronize()
    assert torch.isnan(buf[G:G + P]).all() and _counter() == before
    without = {k: o.clone() for k, o in outs.items()}
    assert all(torch.isfinite(o).all() for o in without.values())
    # the call with the block, both modes
    want = _operator_two_calls("ragged", "values", True)
    for values in (v.data_ptr(), None):
        fresh()
        assert call(args(full, block(values=values))) == 0
        torch.cuda.synchronize()
        assert bool((buf[:G] == 7.0).all()) and bool((buf[-G:] == 9.0).all()) and torch.isfinite(buf).all()
        assert rel_err(buf[G:G + P].double().cpu().numpy(), want["values"]) <= GRAD_BAR
        assert rel_err(outs["color"].cpu().numpy(), without["color"].cpu().numpy()) <= ORDER_BAR   # record slots 0..2 are the image's alone
        assert rel_err(outs["mean2D"].double().cpu().numpy(), want["means2D"]) <= GRAD_BAR
    assert _counter() == before + 2
    # R = 0: dL_dvalues zero-filled, no walk
    fresh()
    assert call(args(full, block(), R=0)) == 0
    torch.cuda.synchronize()
    assert not buf[G:G + P].any() and bool((buf[:G] == 7.0).all()) and bool((buf[-G:] == 9.0).all()) and _counter() == before + 2
    assert _C.profile_read().keys() >= {"render_depth_backward"}


@pytest.mark.gpu
def test_a_captured_backward_call_replays_the_uncaptured_gradients():
    from diff_gaussian_rasterization import _C
    sc = _scene("ragged")
    rs = make_settings(sc["cam"], 0, bg=np.array(BG, np.float32), subpixel_offset=sc["so"])
    t = {k: to_dev(a) for k, a in sc["cloud"].items()}
    dL, dLd = to_dev(sc["cot"]), to_dev(sc["cot_d"])
    frame = _native_frame(_C, rs, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up on the capture stream; the first call also consumes the frame's clean-record mark
            want = _native_backward(_C, rs, t, frame, dL, depth=(dLd, "distance"))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _native_backward(_C, rs, t, frame, dL, depth=(dLd, "distance"))
    for _ in range(2):   # a replay starts from a record it clears itself: the second gives the first's gradients, not their double
        graph.replay()
    torch.cuda.synchronize()
    for k, a, b in zip(NATIVE_NAMES + ("values",), got, want):
        if a is not None and a.numel():
            assert torch.isfinite(a).all(), k
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= ORDER_BAR, k
    assert float(got[8].abs().max()) > 0


# ---- 9. what needs no device ----------------------------------------------------------------------------------------------------------------
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
        p = inspect.signature(fn).parameters["depth_grad"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    # (colour_only, options = (exact, deterministic, record), fixed capacity)
    assert not _C.depth_grad_refused(False, (1, 0, 1)) and not _C.depth_grad_refused(False, (0, 0, 1), False)
    for bad in ((True, (1, 0, 1)), ("fixed_order", (1, 0, 1)), (False, (1, 1, 1)), (False, (1, 0, 0)), (False, (1, 0, 1), True)):
        assert _C.depth_grad_refused(*bad), bad
    for source in ("distance", torch.zeros(5)):
        for kw in (dict(colour_gradients_only=True), dict(colour_gradients_only="fixed_order"), dict(deterministic_backward=True), dict(grad_record=False),
                   dict(binning_capacity=100)):
            with pytest.raises(Exception) as info:   # refused at forward time, before anything is rendered
                _cpu_call(return_depth=source, depth_grad=True, **kw)
            assert str(info.value) == _C.DEPTH_GRAD_MSG, kw
    with pytest.raises(Exception, match="pass return_depth too"):
        _cpu_call(depth_grad=True)
    with pytest.raises(Exception, match="return_depth must be"):
        _cpu_call(return_depth="nearest", depth_grad=True)
    # the block's own checks (the ctypes binding's; the compiled one restates them)
    cot = torch.zeros(3, 4, 6)
    for block, msg in (((torch.zeros(4, 6),), _C.DEPTH_GRAD_BLOCK_MSG), ("distance", _C.DEPTH_GRAD_BLOCK_MSG), ((torch.zeros(4, 5), "distance"), _C.DEPTH_GRAD_COTANGENT_MSG),
                       ((torch.zeros(4, 6, dtype=torch.float64), "distance"), _C.DEPTH_GRAD_COTANGENT_MSG), ((None, "distance"), _C.DEPTH_GRAD_COTANGENT_MSG),
                       ((torch.zeros(4, 6), "nearest"), _C.DEPTH_SOURCE_MSG), ((torch.zeros(4, 6), torch.zeros(4)), "depth values must have P elements")):
        with pytest.raises(RuntimeError) as info:
            _C._check_depth_grad_arguments(block, 5, cot)
        assert str(info.value) == msg, block
    _C._check_depth_grad_arguments((torch.zeros(4, 6), "distance"), 5, cot)


def test_output_and_cotangent_arity_without_a_device(monkeypatch):
    """The native module is replaced by stand-ins: only the tuple logic of the autograd function runs.  depth_grad=False keeps depth
    non-differentiable; with True the depth cotangent reaches the native backward call as the `depth` block with the frame's source, in whichever
    place the outputs put it (fourth, or fifth behind a second image), a None cotangent sends no block, and a loss on depth alone runs the call
    on a zero image cotangent."""
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import _C
    calls = []

    def fake_forward(*a, colors2=None, **kw):
        e = torch.empty(0, dtype=torch.uint8)
        return (7, torch.zeros(3, 4, 6), torch.zeros(5, dtype=torch.int32), e, e, e) + ((torch.ones(3, 4, 6),) if colors2 is not None else ())

    def fake_depth(geom, binning, img, R, P, H, W, source, *a, **kw):
        return torch.full((H, W), 2.0)

    def fake_backward(*a, depth=None, dL_dout_color2=None, **kw):
        dL = a[14]
        calls.append(dict(depth=depth, dL=dL.clone(), second=dL_dout_color2 is not None))
        P = 5
        out = (torch.ones(P, 3), torch.ones(P, 3), torch.ones(P, 1), torch.ones(P, 3), None, torch.zeros(P, 0, 3), torch.ones(P, 3), torch.ones(P, 4))
        if dL_dout_color2 is not None:
            out += (torch.ones(P, 3),)
        return out + ((torch.full((P,), 3.0),) if depth is not None else ())
    monkeypatch.setattr(_C, "rasterize_gaussians", fake_forward)
    monkeypatch.setattr(_C, "render_depth", fake_depth)
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", fake_backward)
    fwd = list(inspect.signature(D._RasterizeGaussians.forward).parameters)
    assert fwd[-2:] == ["depth_grad", "return_depth"]

    def leaves():
        return dict(means3D=torch.zeros(5, 3, requires_grad=True), opacities=torch.ones(5, 1, requires_grad=True))
    # False / absent: four outputs, depth takes no gradient
    for kw in (dict(), dict(depth_grad=False)):
        out = _cpu_call(return_depth="distance", **leaves(), **kw)
        assert len(out) == 4 and out[0].requires_grad and not out[-1].requires_grad
    # True, distance: the cotangent arrives with the source; means3D's gradient is the native call's (the direct term is folded in there)
    t = leaves()
    out = _cpu_call(return_depth="distance", depth_grad=True, **t)
    assert len(out) == 4 and out[-1].requires_grad
    (out[-1] * 0.5).sum().backward()
    assert len(calls) == 1 and calls[0]["depth"][1] == "distance" and torch.equal(calls[0]["depth"][0], torch.full((4, 6), 0.5))
    assert not calls[0]["dL"].any() and calls[0]["dL"].shape == (3, 4, 6) and not calls[0]["second"]   # a zero image cotangent
    assert torch.equal(t["means3D"].grad, torch.ones(5, 3))
    # True, a tensor that requires grad: its gradient is the last element of the native result
    t, values = leaves(), torch.zeros(5, requires_grad=True)
    out = _cpu_call(return_depth=values, depth_grad=True, **t)
    (out[0].sum() + out[-1].sum()).backward()
    assert len(calls) == 2 and calls[1]["depth"][1].shape == (5,) and not calls[1]["depth"][1].requires_grad and bool(calls[1]["dL"].all())
    assert torch.equal(values.grad, torch.full((5,), 3.0))
    # a tensor that takes no gradient gets none
    t, values = leaves(), torch.zeros(5)
    out = _cpu_call(return_depth=values, depth_grad=True, **t)
    out[-1].sum().backward()
    assert len(calls) == 3 and values.grad is None
    # a loss that does not use depth: no block
    t = leaves()
    out = _cpu_call(return_depth="distance", depth_grad=True, **t)
    out[0].sum().backward()
    assert len(calls) == 4 and calls[3]["depth"] is None
    # behind a second image: (color, radii, accumulation, color2, depth)
    t = leaves()
    out = _cpu_call(return_depth="distance", depth_grad=True, colors_precomp2=torch.ones(5, 3), **t)
    assert len(out) == 5 and out[-1].requires_grad
    out[-1].sum().backward()
    assert len(calls) == 5 and calls[4]["depth"] is not None and calls[4]["second"] and torch.equal(calls[4]["depth"][0], torch.ones(4, 6))
