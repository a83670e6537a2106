"""The colour-only backward pass in a fixed summation order (wg_backward_args::colour_gradients_only = 2, `colour_gradients_only="fixed_order"`;
csrc/colour_bwd/fixed_order.hip): the atomic pass's per-tile terms, stored into per-instance slots and added per Gaussian in an order the frame
fixes -- the same bits whatever the schedule.

Bars.  Between two runs, launch orders, bindings and binning paths: torch.equal.  Against the per-tile terms P_t[g, c] (the atomic pass with the
cotangent zeroed outside tile t: every other tile adds an exact +0.0, so the result IS the tile's wave-reduced term): with n the number of
non-zero terms of an element, n <= 1: equal to the term or +0.0; n == 2: equal to their float32 sum; any n:
|g - S| <= (n - 1) u / (1 - (n - 1) u) * sum |P_t| with u = 2^-24 and S the float64 sum -- the a-priori bound of ANY order of n float32
additions, so it is derived and not measured.  Against the float64 oracle: 1e-3 max-rel-err, tests/test_colour_backward.py's bar."""
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
FIXED = "fixed_order"
U = 2.0 ** -24
ORDER_BAR = 2e-6   # two orders of the same float32 sums, relative to the array's largest magnitude (docs/OPTIONS.md): only where the ATOMIC pass is one side


# ---- scenes (numpy clouds) and native calls -------------------------------------------------------------------------------------------------
def _f32(cloud):
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in cloud.items()}


def _concat(a, b):
    return {k: np.concatenate([a[k], b[k]], axis=0) for k in a}


def _wide(n, W, H, seed, opacity=0.05):
    """n Gaussians near the optical axis whose 3-sigma extent is larger than the image: each covers every tile."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 8.0, size=n)
    means = np.stack([0.05 * z * rng.uniform(-1, 1, size=n), 0.05 * z * rng.uniform(-1, 1, size=n), z], axis=1)
    scales = (0.8 * z)[:, None] * np.ones((n, 3))   # ~0.8 / tan(30 deg) * W / 2 pixels of standard deviation: more than the image
    q = np.tile(np.array([1.0, 0, 0, 0]), (n, 1))
    return _f32(dict(means3D=means, scales=scales, rotations=q, opacities=np.full((n, 1), opacity), colors_precomp=rng.uniform(0, 1, size=(n, 3))))


def _multi_tile():
    """48 x 48 (3 x 3 tiles), 300 Gaussians: 290 of the project's recipe at a scale that spreads them over 1 - 6 tiles, 10 that cover all 9."""
    W = H = 48
    return _concat(S.make_cloud(290, W, H, sh_degree=None, seed=7, scale_mult=25.0), _wide(10, W, H, 70)), S.make_camera(W, H), S.make_cotangent(W, H)


def _one_tile(P):
    """One 16 x 16 tile, P faint Gaussians that all cover it (tests/test_render_depth.py: _one_tile): every pixel blends every instance and
    nothing saturates, so the walk's batches end exactly where the list does, and every Gaussian owns one slot."""
    rng = np.random.default_rng(P)
    z = rng.uniform(2.0, 8.0, size=P)
    means = np.stack([0.02 * z * rng.uniform(-1, 1, size=P), 0.02 * z * rng.uniform(-1, 1, size=P), z], axis=1)
    scales = (1.5 * z)[:, None] * np.ones((P, 3))
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    cloud = dict(means3D=means, scales=scales, rotations=q, opacities=np.full((P, 1), 0.01), colors_precomp=rng.uniform(0, 1, size=(P, 3)))
    return _f32(cloud), S.make_camera(16, 16), S.make_cotangent(16, 16)


def _reduce_edges(P):
    """64 x 48 (12 tiles), P Gaussians of the project's recipe over a few tiles each; every fifth one behind the camera (tiles_touched = 0)
    and every seventh one too faint to be blended anywhere (opacity below 1 / 255: it owns slots, none of them is ever flagged)."""
    W, H = 64, 48
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=100 + P, scale_mult=30.0)
    i = np.arange(P)
    culled, faint = (i % 5 == 3), (i % 7 == 5) & (i % 5 != 3)
    cloud["means3D"][culled, 2] *= -1.0
    cloud["opacities"][faint] = 0.002
    return cloud, S.make_camera(W, H), S.make_cotangent(W, H), culled, faint


def _cover_all():
    """64 x 48 (12 tiles), 70 Gaussians that each cover every tile: the first wave's 64 Gaussians own 768 slots, three 256-slot flag fetches."""
    W, H = 64, 48
    return _wide(70, W, H, 71, opacity=0.03), S.make_camera(W, H), S.make_cotangent(W, H)


class Frame:
    """A native forward frame of (cloud, cam) kept for backward calls under the current binding."""

    def __init__(self, _C, cloud, cam, cot, exact=1, bg=(0.2, 0.5, 0.8), so=None):
        self._C, self.exact = _C, int(exact)
        self.P, self.W, self.H = cloud["means3D"].shape[0], cam["width"], cam["height"]
        self.rs = make_settings(cam, 0, bg=np.array(bg, np.float32), subpixel_offset=so)
        self.t = {k: to_dev(v) for k, v in cloud.items()}
        self.dL = to_dev(cot)
        e, rs, t = torch.Tensor([]), self.rs, self.t
        self.frame = _C.rasterize_gaussians(rs.bg, t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix,
                                            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width, e, 0,
                                            rs.campos, False, False, options=dict(exact_compositing=self.exact))
        self.R = int(self.frame[0])

    def views(self):
        return dict(geometry=self._C.view_geometry(self.frame[3], self.P), image=self._C.view_image(self.frame[5], self.H, self.W))

    def backward(self, mode, dL=None, sh=None, **kw):
        e, rs, t, f = torch.Tensor([]), self.rs, self.t, self.frame
        kw.setdefault("options", dict(exact_compositing=self.exact))
        return self._C.rasterize_gaussians_backward(rs.bg, t["means3D"], f[2], t["colors_precomp"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                    rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, self.dL if dL is None else dL,
                                                    e if sh is None else sh, 0, rs.campos, f[3], f[0], f[4], f[5], False, colour_gradients_only=mode, **kw)

    def grad(self, mode, dL=None):
        res = self.backward(mode, dL)
        assert len(res) == 8 and all(r is None for i, r in enumerate(res) if i != 1) and res[1].shape == (self.P, 3)
        return res[1]

    def tile_terms(self):
        """[tiles, P, 3]: the atomic pass with the cotangent zeroed outside one tile -- that tile's wave-reduced terms, bit for bit."""
        out = []
        for ty in range((self.H + 15) // 16):
            for tx in range((self.W + 15) // 16):
                m = torch.zeros_like(self.dL)
                m[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = self.dL[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
                out.append(self.grad(True, m))
        return torch.stack(out)


def hold_to_tile_terms(g, terms):
    """The three requirements of the module docstring; -> (largest |g - S| / bound over the elements with n >= 2, the largest n)."""
    g, terms = g.cpu().numpy(), terms.cpu().numpy()
    assert g.dtype == np.float32 and terms.dtype == np.float32 and np.isfinite(g).all() and np.isfinite(terms).all()
    nz = terms != 0
    n = nz.sum(axis=0)
    # the non-zero terms first, in tile order (a stable sort of "is zero")
    idx = np.argsort(~nz, axis=0, kind="stable")
    first, second = np.take_along_axis(terms, idx[:1], axis=0)[0], (np.take_along_axis(terms, idx[1:2], axis=0)[0] if terms.shape[0] > 1 else np.zeros_like(g))
    none, one, two = n == 0, n == 1, n == 2
    assert not g[none].any() and not np.signbit(g[none]).any()        # an exact +0.0
    assert np.array_equal(g[one], first[one])
    assert np.array_equal(g[two], (first + second)[two])              # float32 addition is commutative
    S64, A64 = terms.astype(np.float64).sum(axis=0), np.abs(terms.astype(np.float64)).sum(axis=0)
    k = np.maximum(n - 1, 0).astype(np.float64)
    bound = k * U / (1.0 - k * U) * A64
    err = np.abs(g.astype(np.float64) - S64)
    assert (err <= bound).all(), float((err - bound).max())
    many = n >= 2
    ratio = float((err[many] / bound[many]).max()) if many.any() else 0.0
    return ratio, int(n.max())


@pytest.fixture()
def binding():
    from diff_gaussian_rasterization import _C
    before = _C.binding_name()
    yield _C
    _C.use_binding(before)


@pytest.fixture()
def options():
    """set_option for the test, the library's defaults back afterwards (tests/test_colour_backward.py: options)."""
    from diff_gaussian_rasterization import _C

    def set_(**kw):
        for k, v in kw.items():
            _C.set_option(k, v)
    yield set_
    set_(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, staged_scatter=-1, force_global_sort=0, geometry_reuse=_C.GEOMETRY_REUSE_DEFAULT,
         backward_order_period=0)


# ---- 1. the same bits whatever the schedule -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
def test_same_bits_under_every_tile_launch_order(options, exact):
    from diff_gaussian_rasterization import _C
    cloud, cam, cot = _multi_tile()
    f = Frame(_C, cloud, cam, cot, exact)
    tt = f.views()["geometry"]["tiles_touched"].cpu().numpy()
    assert f.P == 300 and (tt == 9).sum() >= 10 and ((tt >= 2) & (tt < 9)).sum() >= 20, np.bincount(tt)   # the premise: Gaussians over 2 .. 9 tiles
    got = []
    for period in (0, 1, 128):
        options(backward_order_period=period)
        got += [f.grad(FIXED), f.grad(FIXED)]
    assert float(got[0].abs().max()) > 0
    assert all(torch.equal(got[0], g) for g in got[1:])


# ---- 2. held to the per-tile terms ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
def test_sum_of_the_per_tile_terms_and_the_float64_oracle(oracle, exact):
    from diff_gaussian_rasterization import _C
    cloud, cam, cot = _multi_tile()
    bg = (0.2, 0.5, 0.8)
    f = Frame(_C, cloud, cam, cot, exact, bg=bg)
    g = f.grad(FIXED)
    ratio, n_max = hold_to_tile_terms(g, f.tile_terms())
    print(f"exact_compositing = {exact}: largest |g - S| / bound = {ratio:.4f}, up to {n_max} terms per element")
    assert n_max >= 3
    o = np.asarray(oracle.run_scene(cloud, cam, sh_degree=0, cotangent=cot, precision="f64", bg=np.array(bg, np.float32), subpixel_offset=None)["grads"]["colors_precomp"])
    e = rel_err(g.cpu().numpy(), o)
    print(f"exact_compositing = {exact}: rel_err against the float64 oracle = {e:.3e}")
    if os.environ.get("WG_WRITE_PROFILES") == "1":
        path = os.path.join(ROOT, "profiles", "colour_backward", "accuracy_fixed_order.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[f"multi_tile_48x48_exact_compositing_{exact}"] = dict(largest_error_over_bound=ratio, most_terms_per_element=n_max, rel_err_f64_oracle=e)
        with open(path, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
    assert e <= 1e-3


# ---- 3. batch edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 200])
def test_batch_edges_on_one_tile(P, exact):
    """Every Gaussian owns one slot: nothing is added to anything, the result is the atomic pass's bit for bit."""
    from diff_gaussian_rasterization import _C
    cloud, cam, cot = _one_tile(P)
    f = Frame(_C, cloud, cam, cot, exact)
    v = f.views()
    assert f.R == P and (v["geometry"]["tiles_touched"] == 1).all()
    if exact:   # the premise: every pixel blended every instance
        assert int(v["image"]["n_contrib"].min()) == P and int(v["image"]["tile_last"][0]) == P
    g = f.grad(FIXED)
    assert torch.equal(g, f.grad(True)) and bool((g != 0).any(dim=1).all())


# ---- 4. reduce-kernel edges, through the C-ABI ----------------------------------------------------------------------------------------------
def _c_abi_fixed(_C, f, value=2, options=None, guard=5, **fields):
    """wg_rasterize_backward_ex called directly with dL_dcolor inside a larger NaN-filled buffer -> (status, [P, 3] view, the whole buffer)."""
    from diff_gaussian_rasterization._abi import _BackwardArgs
    buf = torch.full((3 * f.P + 2 * guard,), float("nan"), device="cuda")
    a = _BackwardArgs()
    a.struct_size = C.sizeof(_BackwardArgs)
    a.P, a.R, a.width, a.height = f.P, f.R, f.W, f.H
    a.scale_modifier, a.tan_fovx, a.tan_fovy, a.kernel_size = 1.0, f.rs.tanfovx, f.rs.tanfovy, f.rs.kernel_size
    a.background, a.subpixel_offset, a.dL_dpix = f.rs.bg.data_ptr(), f.rs.subpixel_offset.data_ptr(), f.dL.data_ptr()
    a.dL_dcolor = buf.data_ptr() + 4 * guard   # (guard = 5 floats: the array is not 16-byte aligned either)
    a.geom_buffer, a.binning_buffer, a.image_buffer = f.frame[3].data_ptr(), f.frame[4].data_ptr(), f.frame[5].data_ptr()
    a.stream = torch.cuda.current_stream().cuda_stream
    a.colour_gradients_only = value
    if options is not None:
        a.options = C.pointer(options)
    for k, v in fields.items():
        setattr(a, k, v)
    status = _C._lib.wg_rasterize_backward_ex(C.byref(a))
    torch.cuda.synchronize()
    return status, buf[guard:guard + 3 * f.P].view(f.P, 3), buf


def _guards_untouched(buf, P, guard=5):
    return bool(torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + 3 * P:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_reduce_edges_culled_and_unflagged_gaussians_and_a_nan_filled_target(P):
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization._abi import _CallOptions
    cloud, cam, cot, culled, faint = _reduce_edges(P)
    f = Frame(_C, cloud, cam, cot)
    tt = f.views()["geometry"]["tiles_touched"].cpu().numpy()
    assert not tt[culled].any() and (P < 7 or (tt[faint] > 0).all()), tt   # the premise: culled ones own no slot, faint ones do
    status, got, buf = _c_abi_fixed(_C, f, options=_CallOptions(1, 0, 1))
    assert status == 0 and _guards_untouched(buf, P)
    assert torch.isfinite(got).all()                                       # every one of the 3 P floats was overwritten
    assert not got[to_dev(culled | faint)].any()                           # nothing flagged: an exact zero
    assert torch.equal(got, f.grad(FIXED))                                 # the binding's call computes the same
    ratio, n_max = hold_to_tile_terms(got, f.tile_terms())
    print(f"P = {P}: largest |g - S| / bound = {ratio:.4f}, up to {n_max} terms per element")
    assert float(got.abs().max()) > 0


@pytest.mark.gpu
def test_a_slot_range_that_crosses_the_flag_fetch():
    from diff_gaussian_rasterization import _C
    cloud, cam, cot = _cover_all()
    f = Frame(_C, cloud, cam, cot)
    tt = f.views()["geometry"]["tiles_touched"].cpu().numpy()
    assert f.P == 70 and (tt == 12).all() and f.R == 840   # the first wave's 64 Gaussians: 768 slots
    status, got, buf = _c_abi_fixed(_C, f)
    assert status == 0 and _guards_untouched(buf, f.P) and torch.isfinite(got).all()
    terms = f.tile_terms()
    assert int((terms != 0).any(dim=2).sum(dim=0).min()) >= 9   # nearly every slot is flagged: full 64-entry batches
    ratio, n_max = hold_to_tile_terms(got, terms)
    print(f"cover-all: largest |g - S| / bound = {ratio:.4f}, up to {n_max} terms per element")
    assert n_max == 12
    # any other non-zero value behaves as 1: the atomic pass
    status, other, _ = _c_abi_fixed(_C, f, value=3)
    assert status == 0 and rel_err(other.cpu().numpy(), got.cpu().numpy()) <= ORDER_BAR


# ---- 5. empty inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", BINDINGS)
def test_no_gaussians_and_nothing_in_front_of_the_camera(binding, name):
    from diff_gaussian_rasterization import GaussianRasterizer
    _C = binding
    _C.use_binding(name)
    cam, cot = S.make_camera(48, 48), to_dev(S.make_cotangent(48, 48))
    rs = make_settings(cam, 0)
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)   # noqa: E731
    c0 = z(0, 3)
    img0 = GaussianRasterizer(rs)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=c0, scales=z(0, 3), rotations=z(0, 4), colour_gradients_only=FIXED)[0]
    img0.backward(cot)
    assert c0.grad is not None and c0.grad.shape == (0, 3)
    cloud = S.make_cloud(301, 48, 48, sh_degree=None, seed=3, scale_mult=20.0)
    cloud["means3D"][:, 2] *= -1.0
    f = Frame(_C, cloud, cam, S.make_cotangent(48, 48))
    assert f.R == 0 and not f.frame[2].any()
    g = f.grad(FIXED)
    assert g.shape == (301, 3) and not g.any()
    status, got, buf = _c_abi_fixed(_C, f)
    assert status == 0 and _guards_untouched(buf, f.P) and not got.any() and torch.isfinite(got).all()


# ---- 6. binning paths -----------------------------------------------------------------------------------------------------------------------
def _dense():
    W, H, P = 320, 200, 30000   # ~1000 instances per tile (tests/test_colour_backward.py: _dense): lists the lazy sort splits at test thresholds
    return S.make_cloud(P, W, H, sh_degree=None, seed=5, scale_mult=7.0), S.make_camera(W, H), S.make_cotangent(W, H)


PATHS = {"global_sort": dict(force_global_sort=1), "lazy_sort": dict(lazy_sort=1, lazy_min_len=256, lazy_target=200, lazy_cap=256)}


@pytest.mark.gpu
def test_every_binning_path_gives_the_same_bits(options):
    """Same sorted lists up to tile_last, same rectangles and tiles_touched: the same terms in the same slots, added in the same order."""
    from diff_gaussian_rasterization import _C
    cloud, cam, cot = _dense()
    base = Frame(_C, cloud, cam, cot, bg=(0, 0, 0))
    rg = base.views()["image"]["ranges"].cpu().numpy().astype(np.int64)
    assert (rg[:, 1] - rg[:, 0]).max() > 600
    want = base.grad(FIXED)
    assert float(want.abs().max()) > 0 and rel_err(want.cpu().numpy(), base.grad(True).cpu().numpy()) <= ORDER_BAR
    for path, kw in PATHS.items():
        options(lazy_sort=1, lazy_min_len=1024, lazy_target=820, lazy_cap=2048, force_global_sort=0)
        options(**kw)
        f = Frame(_C, cloud, cam, cot, bg=(0, 0, 0))
        assert torch.equal(f.frame[1], base.frame[1]), path
        assert torch.equal(f.grad(FIXED), want), path


# ---- 7. the operator surface ----------------------------------------------------------------------------------------------------------------
def _step(cloud, cam, cot, mode, colors=None, **fwd):
    """One forward + backward step through the operator -> (image, name -> .grad or None)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = make_settings(cam, 0, bg=np.array((0.2, 0.5, 0.8), np.float32))
    t = {k: to_dev(v).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    if mode is not None:
        fwd["colour_gradients_only"] = mode
    color = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                                   rotations=t["rotations"], **fwd)[0]
    color.backward(to_dev(cot))
    return color.detach(), dict(means2D=m2d.grad, **{k: v.grad for k, v in t.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("name", BINDINGS)
def test_keyword_context_manager_and_a_recolor_frame(binding, options, name):
    _C = binding
    _C.use_binding(name)
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import GaussianRasterizer
    cloud, cam, cot = _multi_tile()
    native = Frame(_C, cloud, cam, cot).grad(FIXED)     # the C-ABI's value 2 through this binding
    _img, by_keyword = _step(cloud, cam, cot, FIXED)
    assert not _C.resolve_colour_gradients_only()
    with D.colour_gradients_only(FIXED):
        assert _C.resolve_colour_gradients_only() == FIXED and _C.resolve_colour_gradients_only(True) is True and _C.resolve_colour_gradients_only(False) is False
        _img, in_block = _step(cloud, cam, cot, None)
    assert _C.resolve_colour_gradients_only() is False
    with D.colour_gradients_only(True):
        assert _C.resolve_colour_gradients_only() is True and _C.resolve_colour_gradients_only(FIXED) == FIXED
    for grads in (by_keyword, in_block):
        assert [k for k, v in grads.items() if v is not None] == ["colors_precomp"]   # the other seven inputs: None
        assert torch.equal(grads["colors_precomp"], native)
    # the second of two calls under geometry_reuse: a recolor frame (its geometry buffer is a child's: rects and tiles_touched copied)
    options(geometry_reuse=1)
    rs = make_settings(cam, 0, bg=np.array((0.2, 0.5, 0.8), np.float32))
    t = {k: to_dev(v).requires_grad_(True) for k, v in cloud.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    geo = dict(means3D=t["means3D"], means2D=m2d, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    hits = _C.geometry_reuse_hits()
    GaussianRasterizer(rs)(colors_precomp=torch.rand(cloud["means3D"].shape[0], 3, device="cuda"), **geo)
    img = GaussianRasterizer(rs)(colors_precomp=t["colors_precomp"], colour_gradients_only=FIXED, **geo)[0]
    assert _C.geometry_reuse_hits() == hits + 1
    img.backward(to_dev(cot))
    options(geometry_reuse=0)
    assert m2d.grad is None and t["means3D"].grad is None
    assert torch.equal(t["colors_precomp"].grad, native)


@pytest.mark.gpu
def test_refused_with_the_atomic_modes_message_under_both_bindings(binding):
    """tests/test_colour_backward.py's refusals with "fixed_order" in place of True: the same calls, the same message."""
    _C = binding
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization._abi import _CallOptions
    assert built, "the compiled binding is not built (python wild-gaussians_amd/build.py --torch-binding): 'both bindings' needs both"
    P, W, H = 2000, 160, 96
    cam = S.make_camera(W, H)
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=3)
    t = {k: to_dev(v) for k, v in cloud.items()}
    shs = to_dev(S.make_cloud(P, W, H, sh_degree=1, seed=3)["shs"])
    rs = make_settings(cam, 1)
    dL = to_dev(S.make_cotangent(W, H))
    ones = torch.ones(P, 3, device="cuda")
    native = dict(shs=dict(sh=shs), sh_mul=dict(sh_tone=(ones, None, None, None)), colors_precomp2=dict(dL_dout_color2=dL),
                  filter_3D=dict(raw=(torch.ones(P, 1, device="cuda"), t["opacities"])), deterministic_backward=dict(options=dict(deterministic_backward=1)))
    base = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    col = dict(colors_precomp=t["colors_precomp"])
    operator = dict(shs=dict(shs=shs), sh_mul=dict(**col, sh_mul=ones), colors_precomp2=dict(**col, colors_precomp2=ones),
                    filter_3D=dict(**col, filter_3D=torch.ones(P, 1, device="cuda")), deterministic_backward=dict(**col, deterministic_backward=True))
    said = {}
    for name in BINDINGS:
        _C.use_binding(name)
        f = Frame(_C, cloud, cam, S.make_cotangent(W, H))
        for case, kw in native.items():
            with pytest.raises(RuntimeError) as info:
                f.backward(FIXED, **kw)
            said[name, "native", case] = str(info.value)
        for case, kw in operator.items():
            with pytest.raises(Exception) as info:
                GaussianRasterizer(rs)(**base, **kw, colour_gradients_only=FIXED)
            said[name, "operator", case] = str(info.value)
        with pytest.raises(ValueError):   # an unknown mode never reaches the library
            f.backward("fixed")
        g = f.grad(FIXED)   # a refused call leaves nothing behind: the well-formed one runs
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert set(said.values()) == {_C.COLOUR_ONLY_MSG}, said
    # the library's own refusals of value 2 (WG_ERR_INVALID_ARGUMENT = -1), nothing written
    for kw in (dict(options=_CallOptions(1, 1, 1)), dict(shs=dL.data_ptr()), dict(options=_CallOptions(0, 0, 1))):   # deterministic_backward; SH colours; a frame
        status, got, buf = _c_abi_fixed(_C, f, **kw)                                                                   # composited with the other arithmetic
        assert status == -1 and torch.isnan(buf).all(), kw


@pytest.mark.gpu
def test_refused_inside_a_stream_capture():
    """The scratch is leased for the call's duration: a captured call is refused before anything is launched, as the full pass's deterministic
    mode is (tests/test_parity_gpu.py: the fixed-capacity forward's capture test, which this follows); the capture itself survives the refusal."""
    from diff_gaussian_rasterization import _C
    W, H, P = 160, 96, 2000
    cam = S.make_camera(W, H)
    static = {k: to_dev(v) for k, v in S.make_cloud(P, W, H, sh_degree=None, seed=3).items()}
    rs, cot, e = make_settings(cam, 0), to_dev(S.make_cotangent(W, H)), torch.Tensor([])
    cap = 200_000

    def forward():
        return _C.rasterize_gaussians(rs.bg, static["means3D"], static["colors_precomp"], static["opacities"], static["scales"], static["rotations"], 1.0, e,
                                      rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, H, W, e, 0, rs.campos, False, False,
                                      None, cap)

    def backward(frame, mode):
        return _C.rasterize_gaussians_backward(rs.bg, static["means3D"], frame[2], static["colors_precomp"], static["scales"], static["rotations"], 1.0, e, rs.viewmatrix,
                                               rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, cot, e, 0, rs.campos, frame[3], frame[0],
                                               frame[4], frame[5], False, colour_gradients_only=mode)
    _C.set_option("geometry_reuse", 0)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):   # warm-up on the capture stream (lazy initialisations, LDS attributes)
                fr = forward()
                want = backward(fr, FIXED)[1]
        torch.cuda.current_stream().wait_stream(side)
        assert _C.forward_status(fr[5], H, W)[1] and float(want.abs().max()) > 0
        g = torch.cuda.CUDAGraph()
        refused = None
        with torch.cuda.graph(g):
            fr = forward()
            try:
                backward(fr, FIXED)
            except RuntimeError as ex:
                refused = str(ex)
        assert refused is not None and "invalid argument" in refused.lower(), refused
        del g
        torch.cuda.synchronize()
        assert torch.equal(backward(forward(), FIXED)[1], want)   # outside a capture the mode works as before
    finally:
        _C.set_option("geometry_reuse", _C.GEOMETRY_REUSE_DEFAULT)


def test_an_unknown_mode_is_a_value_error_without_a_device():
    import diff_gaussian_rasterization as D
    import wg_integration
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    assert _C.resolve_colour_gradients_only(FIXED) == FIXED and _C.resolve_colour_gradients_only(True) is True
    assert _C.resolve_colour_gradients_only(False) is False and _C.resolve_colour_gradients_only() is False
    P = 5
    rs = GaussianRasterizationSettings(image_height=4, image_width=6, tanfovx=1.0, tanfovy=1.0, kernel_size=0.1, subpixel_offset=torch.zeros(4, 6, 2),
                                       bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False, return_accumulation=False)
    cpu = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1), colors_precomp=torch.ones(P, 3), scales=torch.ones(P, 3),
               rotations=torch.ones(P, 4))
    e = torch.Tensor([])
    for bad in ("fixed", "Fixed_Order", "", "deterministic"):
        with pytest.raises(ValueError, match="colour_gradients_only"):
            _C.resolve_colour_gradients_only(bad)
        with pytest.raises(ValueError, match="colour_gradients_only"):
            with D.colour_gradients_only(bad):
                pass
        assert _C.resolve_colour_gradients_only() is False   # the refused block changed nothing
        with pytest.raises(ValueError, match="colour_gradients_only"):
            GaussianRasterizer(rs)(**cpu, colour_gradients_only=bad)
        with pytest.raises(ValueError, match="colour_gradients_only"):
            D.rasterize_gaussians(cpu["means3D"], cpu["means2D"], e, cpu["colors_precomp"], cpu["opacities"], cpu["scales"], cpu["rotations"], e, rs,
                                  colour_gradients_only=bad)
        with pytest.raises(ValueError, match="colour_gradients_only"):
            _C.rasterize_gaussians_backward(rs.bg, cpu["means3D"], e, cpu["colors_precomp"], cpu["scales"], cpu["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                            1.0, 1.0, 0.1, rs.subpixel_offset, torch.zeros(3, 4, 6), e, 0, rs.campos, e, 0, e, e, False, colour_gradients_only=bad)
    # the caller opt-in: "fixed_order" wraps optimize_embedding in the fixed-order default, True in the atomic one, anything else is refused
    seen = []

    class WildGaussians:
        def optimize_embedding(self, dataset, *, embedding=None):
            seen.append(_C.resolve_colour_gradients_only())
            return dict(embedding=embedding, dataset=dataset)

    fake = types.SimpleNamespace(WildGaussians=WildGaussians, GaussianModel=type("GaussianModel", (), {}))
    original = WildGaussians.optimize_embedding
    off = dict(ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False)
    undo = wg_integration.apply_optins(fake, embedding_optim=FIXED, **off)
    assert WildGaussians().optimize_embedding("d", embedding=3) == dict(embedding=3, dataset="d")
    undo()
    assert WildGaussians.optimize_embedding is original
    undo = wg_integration.apply_optins(fake, embedding_optim=True, **off)
    WildGaussians().optimize_embedding("d")
    undo()
    WildGaussians().optimize_embedding("d")
    assert seen == [FIXED, True, False] and _C.resolve_colour_gradients_only() is False
    with pytest.raises(ValueError, match="embedding_optim"):
        wg_integration.apply_optins(fake, embedding_optim="fixed", **off)
    assert WildGaussians.optimize_embedding is original


# ---- 8. the loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_embedding_fits_end_at_the_same_bits():
    import appearance_colour_lib as L
    import wg_fused_gaussians as FG
    from diff_gaussian_rasterization import GaussianRasterizer
    P, Wd, H, G, E = 200, 32, 32, 24, 32
    cam = S.make_camera(Wd, H)
    cloud = S.make_cloud(P, Wd, H, sh_degree=None, seed=5, scale_mult=12.0)
    rast = GaussianRasterizer(make_settings(cam, 3))
    gen = torch.Generator().manual_seed(9)
    t = dict(means3D=to_dev(cloud["means3D"]), opacities=to_dev(cloud["opacities"]), scales=to_dev(cloud["scales"]), rotations=to_dev(cloud["rotations"]),
             features=(torch.rand(P, 48, generator=gen) * 1.75 - 0.25).cuda(), gembedding=(torch.rand(P, G, generator=gen) * 2 - 1).cuda())
    Wt = L.draw_weights(3 + G + E, 17)
    Wt[0][:, 3 + G:] *= 6
    Wt[4] = Wt[4] * 40
    weights = [w.cuda() for w in Wt]
    emb0, emb_gt = (torch.randn(E, generator=gen) * 0.3).cuda(), (torch.randn(E, generator=gen) * 0.3).cuda()
    with torch.no_grad():
        col = FG.toned_colours(t["features"], t["gembedding"], emb_gt, t["means3D"], rast.raster_settings.campos, weights, 3)
        gt = rast(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], colors_precomp=col, scales=t["scales"],
                  rotations=t["rotations"])[0]
    args = (rast, t["means3D"], t["opacities"], t["scales"], t["rotations"], t["features"], t["gembedding"], weights, emb0, gt)
    a, b = FG.fit_appearance_embedding(*args, iters=4, fixed_order=True), FG.fit_appearance_embedding(*args, iters=4, fixed_order=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], emb0) and a[1].shape == (4,) and a[2].shape == (4,)
    d = FG.fit_appearance_embedding(*args, iters=4)   # the atomic mode: the same sums in another order (nothing is asserted about its own spread)
    for i in range(4):
        assert abs(float(a[1][i]) - float(d[1][i])) <= 1e-5 * abs(float(d[1][i])), (i, float(a[1][i]), float(d[1][i]))
