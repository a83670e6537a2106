"""The colour-only backward pass (wg_backward_args::colour_gradients_only; csrc/render_bwd.hip: render_backward_colour_kernel): dL_dcolors of a frame with
precomputed colours from one front-to-back walk that sums the forward pass's own blend weights, and nothing else.

Bars: 1e-3 max-rel-err against the float32 oracle (the project's gradient bar); against the float64 oracle and against the identity
sum_g <dL_dcolors[g], colors[g]> = <cotangent, image> at most twice the full backward pass's own error on the same frame; 2e-6 of the
array's largest magnitude between two orders of the same sums (docs/OPTIONS.md)."""
import ctypes as C
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

import wg_scenes as S
from wg_testlib import make_settings, rel_err, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = bool(glob.glob(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "_C_torch*.so")))
BINDINGS = ["torch", "ctypes"]

# name: P, W, H, scale_mult, random sub-pixel offsets, background   (tests/test_parity_gpu.py: CASES, with precomputed colours)
SCENES = {
    "ragged": (8000, 250, 130, 3.0, True, (0.2, 0.5, 0.8)),       # partial tiles
    "saturating": (1500, 320, 200, 12.0, False, (0.1, 0.3, 0.2)),  # long lists, pixels that stop early through n_contrib
    "plain": (10000, 256, 256, 1.0, False, (0.1, 0.3, 0.2)),
}
ORDER_BAR = 2e-6   # two orders of the same float32 sums (docs/OPTIONS.md)


def _scene(name, zero_bg=False):
    P, W, H, sm, offsets, bg = SCENES[name]
    cam = S.make_camera(W, H)
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=11, scale_mult=sm)
    so = np.random.default_rng(3).uniform(-0.5, 0.5, size=(H, W, 2)).astype(np.float32) if offsets else None
    return cloud, cam, dict(bg=np.zeros(3, np.float32) if zero_bg else np.array(bg, np.float32), subpixel_offset=so), S.make_cotangent(W, H)


def _step(cloud, cam, kw, cot, colour_only, colors=None, **fwd):
    """One forward + backward step through the operator -> dict(color, radii, grads: name -> array or None)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=kw["bg"], subpixel_offset=kw["subpixel_offset"])
    t = {k: to_dev(v).requires_grad_(True) for k, v in cloud.items()}
    if colors is not None:
        t["colors_precomp"] = colors
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    if colour_only is not None:
        fwd["colour_gradients_only"] = colour_only
    color, radii, _acc = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], colors_precomp=t["colors_precomp"],
                                                scales=t["scales"], rotations=t["rotations"], **fwd)
    color.backward(to_dev(cot))
    grads = dict(means2D=m2d.grad, **{k: v.grad for k, v in t.items()})
    return dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(),
                grads={k: None if g is None else g.detach().cpu().numpy() for k, g in grads.items()})


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def flagged(name, zero_bg=False, exact=True):
    """(exact = False: exact_compositing = 0, the kernel's instance on the fast alpha evaluator)"""
    return _cached(("flag", name, zero_bg, exact), lambda: _step(*_scene(name, zero_bg), True, **({} if exact else {"exact_compositing": False})))


def full(name, zero_bg=False):
    return _cached(("full", name, zero_bg), lambda: _step(*_scene(name, zero_bg), False))


def oracle_grad(oracle, name, precision):
    def make():
        cloud, cam, kw, cot = _scene(name)
        o = oracle.run_scene(cloud, cam, sh_degree=0, cotangent=cot, precision=precision, **kw)
        return dict(colors=np.asarray(o["grads"]["colors_precomp"]), radii=np.asarray(o["radii"]))
    return _cached(("oracle", name, precision), make)


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)


@pytest.fixture()
def options():
    """set_option for the test, the library's defaults back afterwards (the way test_parity_gpu.py's lazy_options does)."""
    from diff_gaussian_rasterization import _C

    def set_(**kw):
        for k, v in kw.items():
            _C.set_option(k, v)
    yield set_
    set_(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, staged_scatter=-1, force_global_sort=0, geometry_reuse=_C.GEOMETRY_REUSE_DEFAULT)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_colour_gradients_match_the_oracle_and_nothing_else_is_returned(oracle, mode, name):
    """mode "fast": exact_compositing = 0 on both calls of the frame -- render_backward_colour_kernel<false> -- at the same bar."""
    h, o = flagged(name, exact=mode == "exact"), oracle_grad(oracle, name, "f32")
    g = h["grads"]["colors_precomp"]
    assert g is not None and g.shape == o["colors"].shape
    e = rel_err(g, o["colors"])
    print(f"{name} / {mode}: rel_err of the colour-only dL_dcolors against the float32 oracle = {e:.3e}")
    assert np.array_equal(h["radii"], o["radii"])
    assert e <= 1e-3
    assert not np.abs(g[o["radii"] == 0]).any()        # exactly zero for culled Gaussians
    assert np.abs(g).max() > 0
    assert all(v is None for k, v in h["grads"].items() if k != "colors_precomp"), [k for k, v in h["grads"].items() if v is not None]


# ---- 2. against the float64 oracle, relative to the full backward pass ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_error_against_float64_is_at_most_twice_the_full_backward_passes(oracle, name):
    ref = oracle_grad(oracle, name, "f64")["colors"]
    e_flag, e_full = rel_err(flagged(name)["grads"]["colors_precomp"], ref), rel_err(full(name)["grads"]["colors_precomp"], ref)
    print(f"{name}: rel_err against the float64 oracle: colour-only {e_flag:.3e}, full backward {e_full:.3e}")
    if os.environ.get("WG_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "colour_backward", "accuracy.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = dict(rel_err_f64_colour_only=e_flag, rel_err_f64_full_backward=e_full)
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    assert e_flag <= 1e-3
    if e_full > 0:
        assert e_flag <= 2 * e_full


# ---- 3. tied to the forward image -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_colour_gradients_reproduce_the_forward_image(name):
    """With a zero background the image is linear in the colours over the blended pairs: sum_g <dL_dcolors[g], colors[g]> = <cotangent, image>.
    A pair the forward pass did not blend, or a blended one missed, breaks it."""
    cloud, _cam, _kw, cot = _scene(name, zero_bg=True)
    h, f = flagged(name, zero_bg=True), full(name, zero_bg=True)
    assert np.array_equal(h["color"], f["color"])
    target = float((cot.astype(np.float64) * h["color"].astype(np.float64)).sum())
    col = cloud["colors_precomp"].astype(np.float64)
    res = {k: abs(float((r["grads"]["colors_precomp"].astype(np.float64) * col).sum()) - target) / abs(target) for k, r in (("flag", h), ("full", f))}
    print(f"{name}: |sum_g <dL_dcolors, colors> - <cotangent, image>| / |<cotangent, image>|: colour-only {res['flag']:.3e}, full backward {res['full']:.3e}")
    assert res["flag"] <= 2 * res["full"]


# ---- 4. the same sums on every binning path -------------------------------------------------------------------------------------------------
def _dense():
    W, H, P = 320, 200, 30000   # ~1000 instances per tile (test_parity_gpu.py: _dense_scene): lists the lazy sort splits at test thresholds
    return S.make_cloud(P, W, H, sh_degree=None, seed=5, scale_mult=7.0), S.make_camera(W, H), dict(bg=np.zeros(3, np.float32), subpixel_offset=None), S.make_cotangent(W, H)


PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256),
         "staged_scatter": dict(staged_scatter=1)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["saturating", "dense"])
def test_every_binning_path_gives_the_same_sums(options, name, path):
    """The walk reads each tile's list up to tile_last only: behind it lie the unsorted tails of lazily sorted lists.  ("dense": lists long
    enough for the lazy sort to engage at these thresholds whatever the first scene's lengths are.)"""
    scene = _dense() if name == "dense" else _scene(name)
    base = _cached(("path-default", name), lambda: _step(*scene, True))   # (the library's defaults: the fixture puts them back after every test)
    options(**PATHS[path])
    got = _step(*scene, True)
    assert np.array_equal(got["color"], base["color"])
    e = rel_err(got["grads"]["colors_precomp"], base["grads"]["colors_precomp"])
    print(f"{name} / {path}: rel_err against the default path = {e:.3e}")
    assert e <= ORDER_BAR
    if name == "dense":
        from wg_testlib import run_hip_native
        cloud, cam, _kw, _cot = scene
        rg = run_hip_native(cloud, cam, sh_degree=0)["views"]["image"]["ranges"].cpu().numpy().astype(np.int64)
        assert (rg[:, 1] - rg[:, 0]).max() > 600


# ---- 5. surface and refusals, both bindings -------------------------------------------------------------------------------------------------
def _native_frame(_C, rs, t, **fwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                  rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0, rs.campos, False, False, **fwd)


def _native_backward(_C, rs, t, frame, dL, sh=None, **bwd):
    e = torch.Tensor([])
    return _C.rasterize_gaussians_backward(rs.bg, t["means3D"], frame[2], t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                           rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, dL, e if sh is None else sh, 0, rs.campos,
                                           frame[3], frame[0], frame[4], frame[5], False, **bwd)


@pytest.mark.gpu
def test_refused_combinations_raise_the_same_message_under_both_bindings(binding):
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    P, W, H = 2000, 160, 96
    cam = S.make_camera(W, H)
    t = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=3).items()}
    shs = to_dev(S.make_cloud(P, W, H, sh_degree=1, seed=3)["shs"])
    rs = make_settings(cam, 1)
    dL = to_dev(S.make_cotangent(W, H))
    ones = torch.ones(P, 3, device="cuda")
    native = dict(shs=dict(sh=shs), sh_mul=dict(sh_tone=(ones, None, None, None)), colors_precomp2=dict(dL_dout_color2=dL),
                  filter_3D=dict(raw=(torch.ones(P, 1, device="cuda"), t["opacities"])), deterministic_backward=dict(options=dict(deterministic_backward=1)))
    base = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    col = dict(colors_precomp=t["colors_precomp"])
    operator = dict(shs=dict(shs=shs), sh_mul=dict(**col, sh_mul=ones), sh_clamp=dict(**col, sh_post_clamp_max=1.0), colors_precomp2=dict(**col, colors_precomp2=ones),
                    filter_3D=dict(**col, filter_3D=torch.ones(P, 1, device="cuda")), deterministic_backward=dict(**col, deterministic_backward=True))
    said = {}
    for name in BINDINGS:
        _C.use_binding(name)
        frame = _native_frame(_C, rs, t)
        for case, kw in native.items():
            with pytest.raises(RuntimeError) as info:
                _native_backward(_C, rs, t, frame, dL, colour_gradients_only=True, **kw)
            said[name, "native", case] = str(info.value)
        for case, kw in operator.items():
            with pytest.raises(Exception) as info:
                GaussianRasterizer(rs)(**base, **kw, colour_gradients_only=True)
            said[name, "operator", case] = str(info.value)
        # a refused call leaves nothing behind: the well-formed one runs, with None in the other seven places
        res = _native_backward(_C, rs, t, frame, dL, colour_gradients_only=True)
        assert len(res) == 8 and all(r is None for i, r in enumerate(res) if i != 1) and res[1].shape == (P, 3) and torch.isfinite(res[1]).all()
    assert set(said.values()) == {_C.COLOUR_ONLY_MSG}, said


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["torch", "ctypes"])
def test_surface_under_each_binding(oracle, binding, options, name):
    """The thread-scoped default, the untouched geometry gradients, frames made by the fixed-capacity forward and by geometry reuse, an odd
    Gaussian count (3 P is no multiple of the float4 the clearing launch writes), no Gaussians, and a cloud that is culled whole."""
    _C = binding
    _C.use_binding(name)
    import diff_gaussian_rasterization as D
    ref, o = flagged("plain"), oracle_grad(oracle, "plain", "f32")
    scene = _scene("plain")
    # the thread's default is seen by a call without the keyword, and is gone after the block
    assert D.colour_gradients_only is _C.colour_gradients_only and not _C.resolve_colour_gradients_only()
    with D.colour_gradients_only(True):
        assert _C.resolve_colour_gradients_only() and not _C.resolve_colour_gradients_only(False)
        inside = _step(*scene, None)
    assert not _C.resolve_colour_gradients_only()
    outside = _step(*scene, None)
    assert inside["grads"]["means2D"] is None and inside["grads"]["means3D"] is None and inside["grads"]["opacities"] is None
    assert all(v is not None for v in outside["grads"].values())
    assert rel_err(inside["grads"]["colors_precomp"], ref["grads"]["colors_precomp"]) <= ORDER_BAR
    # a fixed-capacity frame
    fixed = _step(*scene, True, binning_capacity=1_000_000)
    assert _C.last_forward_status()[1]
    assert rel_err(fixed["grads"]["colors_precomp"], ref["grads"]["colors_precomp"]) <= ORDER_BAR and rel_err(fixed["grads"]["colors_precomp"], o["colors"]) <= 1e-3
    # a frame rendered through geometry reuse: the second of two calls over identical geometry
    from diff_gaussian_rasterization import GaussianRasterizer
    cloud, cam, kw, cot = scene
    options(geometry_reuse=1)
    rs = make_settings(cam, 0, bg=kw["bg"])
    t = {k: to_dev(v).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    other = torch.rand(cloud["means3D"].shape[0], 3, device="cuda")
    geo = dict(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    hits = _C.geometry_reuse_hits()
    GaussianRasterizer(rs)(colors_precomp=other, **geo)
    img = GaussianRasterizer(rs)(colors_precomp=t["colors_precomp"], colour_gradients_only=True, **geo)[0]
    assert _C.geometry_reuse_hits() == hits + 1
    img.backward(to_dev(cot))
    options(geometry_reuse=0)
    reused = t["colors_precomp"].grad.cpu().numpy()
    assert m2d.grad is None and t["means3D"].grad is None
    assert rel_err(reused, ref["grads"]["colors_precomp"]) <= ORDER_BAR and rel_err(reused, o["colors"]) <= 1e-3
    # an odd count
    P, W, H = 2001, 160, 96
    odd = (S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=3.0), S.make_camera(W, H), dict(bg=np.array([0.3, 0.1, 0.6], np.float32), subpixel_offset=None),
           S.make_cotangent(W, H))
    oo = oracle.run_scene(odd[0], odd[1], sh_degree=0, cotangent=odd[3], bg=odd[2]["bg"])
    assert rel_err(_step(*odd, True)["grads"]["colors_precomp"], oo["grads"]["colors_precomp"]) <= 1e-3
    # no Gaussians; a cloud behind the camera
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    c0 = z(0, 3)
    img0 = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=c0, scales=z(0, 3), rotations=z(0, 4), colour_gradients_only=True)[0]
    img0.backward(to_dev(cot))
    assert c0.grad is not None and c0.grad.shape == (0, 3)
    behind = dict(odd[0], means3D=odd[0]["means3D"] * np.array([1, 1, -1], np.float32))
    culled = _step(behind, *odd[1:], True)
    assert not culled["radii"].any() and culled["grads"]["colors_precomp"].shape == (P, 3) and not culled["grads"]["colors_precomp"].any()
    assert culled["grads"]["means2D"] is None


# ---- 6. the C-ABI, without torch in the call ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "odd"])
def test_c_abi_overwrites_dl_dcolor_and_an_older_struct_gets_the_full_pass(oracle, name):
    """wg_rasterize_backward_ex called directly: every output pointer but dL_dcolor NULL, dL_dcolor full of NaN on entry, the flag set -> the
    result of the operator ("overwrites its outputs"; "odd": 3 P is no multiple of four floats, and nothing behind the array is touched).  The
    same struct declared 312 bytes long (version 0.5's layout) hides the flag: the full pass runs and refuses its NULL outputs."""
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _BackwardArgs, _CallOptions
    from wg_testlib import run_hip_native
    if name == "plain":
        cloud, cam, kw, cot = _scene("plain")
        want = flagged("plain")["grads"]["colors_precomp"]
    else:
        P, W, H = 2001, 160, 96
        cloud, cam, kw, cot = (S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=3.0), S.make_camera(W, H),
                               dict(bg=np.array([0.3, 0.1, 0.6], np.float32), subpixel_offset=None), S.make_cotangent(W, H))
        want = np.asarray(oracle.run_scene(cloud, cam, sh_degree=0, cotangent=cot, bg=kw["bg"])["grads"]["colors_precomp"])
    P, W, H = cloud["means3D"].shape[0], cam["width"], cam["height"]
    n = run_hip_native(cloud, cam, sh_degree=0, **kw)
    gb, bb, ib = n["buffers"]
    rs = make_settings(cam, 0, bg=kw["bg"], subpixel_offset=kw["subpixel_offset"])
    dL = to_dev(cot)
    out = torch.full((3 * P + 4,), float("nan"), device="cuda")

    def args(struct_size, options=None):
        a = _BackwardArgs()
        a.struct_size = struct_size
        a.P, a.R, a.width, a.height = P, int(n["num_rendered"]), W, H
        a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, rs.tanfovx, rs.tanfovy, rs.kernel_size
        a.background, a.subpixel_offset, a.dL_dpix, a.dL_dcolor = rs.bg.data_ptr(), rs.subpixel_offset.data_ptr(), dL.data_ptr(), out.data_ptr()
        a.geom_buffer, a.binning_buffer, a.image_buffer = gb.data_ptr(), bb.data_ptr(), ib.data_ptr()
        a.stream = torch.cuda.current_stream().cuda_stream
        a.colour_gradients_only = 1
        if options is not None:
            a.options = C.pointer(options)
        return a
    assert C.sizeof(_BackwardArgs) > 312
    assert _C._lib.wg_rasterize_backward_ex(C.byref(args(312))) == -1            # the tail read as absent: the full pass, which needs its outputs
    det = _CallOptions(1, 1, 1)
    assert _C._lib.wg_rasterize_backward_ex(C.byref(args(C.sizeof(_BackwardArgs), det))) == -1   # no slot path for three sums
    shs = args(C.sizeof(_BackwardArgs))
    shs.shs = dL.data_ptr()
    assert _C._lib.wg_rasterize_backward_ex(C.byref(shs)) == -1                 # SH colours have per-Gaussian work behind dL_dcolor
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                               # a refused call writes nothing
    assert _C._lib.wg_rasterize_backward_ex(C.byref(args(C.sizeof(_BackwardArgs)))) == 0
    torch.cuda.synchronize()
    got = out[:3 * P].view(P, 3).cpu().numpy()
    assert torch.isnan(out[3 * P:]).all()
    assert np.isfinite(got).all()
    assert rel_err(got, want) <= (ORDER_BAR if name == "plain" else 1e-3)


# ---- 7. the caller opt-in (no GPU) ----------------------------------------------------------------------------------------------------------
def test_embedding_optim_optin_wraps_optimize_embedding_in_the_thread_default():
    import wg_integration
    from diff_gaussian_rasterization import _C
    seen = []

    class WildGaussians:
        def optimize_embedding(self, dataset, *, embedding=None):
            seen.append(_C.resolve_colour_gradients_only())
            return dict(embedding=embedding, dataset=dataset)

    fake = types.SimpleNamespace(WildGaussians=WildGaussians, GaussianModel=type("GaussianModel", (), {}))
    original = WildGaussians.optimize_embedding
    off = dict(ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False)
    undo = wg_integration.apply_optins(fake, **off)   # off by default
    assert WildGaussians.optimize_embedding is original
    undo()
    undo = wg_integration.apply_optins(fake, embedding_optim=True, **off)
    assert WildGaussians.optimize_embedding is not original
    assert WildGaussians().optimize_embedding("d", embedding=3) == dict(embedding=3, dataset="d")
    assert seen == [True] and not _C.resolve_colour_gradients_only()
    undo()
    assert WildGaussians.optimize_embedding is original
    with pytest.raises(ValueError, match="edited_module"):   # the edited render makes calls the colour-only pass refuses
        wg_integration.apply_optins(fake, embedding_optim=True, edited_module=types.SimpleNamespace(), **off)
    assert WildGaussians.optimize_embedding is original
    WildGaussians().optimize_embedding("d")
    assert seen == [True, False]
