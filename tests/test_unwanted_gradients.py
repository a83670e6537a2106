"""Gradients nobody asked for are not stored: with SH colours and the gradient record dL_dcolors is an intermediate (already applied to dL_dsh),
with scales and rotations dL_dcov3D is one (already applied to dL_dscales / dL_drotations).  wg_backward_args::dL_dcolor / dL_dcov3D may then be
NULL -- the per-Gaussian kernel skips the stores -- and both bindings take a `want` indication: what is not wanted is neither allocated nor
handed over and comes back as None.  The autograd function passes the needs_input_grad of `colors_precomp` and `cov3D_precomp`; the low-level
call keeps returning all eight by default.

Bit comparisons run under deterministic_backward = 1; oracle comparisons use the bound of tests/test_backward_row.py (1e-3 max-rel-err)."""
import numpy as np
import pytest
import torch

import wg_scenes as S
from wg_testlib import compare_grads, make_settings, to_dev

GRAD_BOUND = 1e-3
W, H, DEG = 64, 48, 3
EIGHT = ("means2D", "colors_precomp", "opacities", "means3D", "cov3Ds_precomp", "sh", "scales", "rotations")
_cases = {}


def _case(P):
    if P not in _cases:
        _cases[P] = (S.make_camera(W, H), S.make_cloud(P, W, H, sh_degree=DEG, seed=3, scale_mult=25.0), S.make_cotangent(W, H))
    return _cases[P]


def _low_level(cloud, cam, cot, deg, binding, **kw):
    """Forward and backward through the native module (the backward call through the named binding) -> the eight-tuple."""
    from diff_gaussian_rasterization import _C
    rs = make_settings(cam, deg)
    e = torch.Tensor([])
    t = {k: to_dev(v) for k, v in cloud.items()}
    opts = dict(deterministic_backward=1)
    R, color, radii, gb, bb, ib = _C.rasterize_gaussians(rs.bg, t["means3D"], t.get("colors_precomp", e), t["opacities"], t.get("scales", e),
                                                         t.get("rotations", e), 1.0, t.get("cov3D_precomp", e), rs.viewmatrix, rs.projmatrix,
                                                         rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, rs.image_height, rs.image_width,
                                                         t.get("shs", e), deg, rs.campos, False, False, options=opts)
    saved = _C._torch_ext
    if binding == "ctypes":
        _C._torch_ext = None
    try:
        return _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, t.get("colors_precomp", e), t.get("scales", e), t.get("rotations", e), 1.0,
                                               t.get("cov3D_precomp", e), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size,
                                               rs.subpixel_offset, to_dev(cot), t.get("shs", e), deg, rs.campos, gb, R, bb, ib, False, options=opts, **kw)[:8]
    finally:
        _C._torch_ext = saved


def _autograd(cloud, cam, cot, deg, grad_keys, monkeypatch, **kw):
    """Through GaussianRasterizer; -> (gradients by wg_testlib name, the `want` the native backward call was given, its eight-tuple)."""
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    seen = {}
    real = _C.rasterize_gaussians_backward

    def spy(*a, **k):
        seen["want"] = k.get("want")
        seen["res"] = real(*a, **k)
        return seen["res"]
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", spy)
    t = {k: to_dev(v).requires_grad_(k in grad_keys) for k, v in cloud.items()}
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    color, _, _ = GaussianRasterizer(make_settings(cam, deg))(means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=t.get("shs"),
                                                              colors_precomp=t.get("colors_precomp"), scales=t.get("scales"), rotations=t.get("rotations"),
                                                              cov3D_precomp=t.get("cov3D_precomp"), **kw)
    color.backward(to_dev(cot))
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", real)
    names = dict(shs="sh", cov3D_precomp="cov3Ds_precomp")
    g = {names.get(k, k): v.grad for k, v in t.items() if v.grad is not None}
    g["means2D"] = means2D.grad
    return g, seen["want"], seen["res"][:8]


def _cov3d_of(cloud):
    """The cloud with its covariances precomputed from scales and rotations (float64, stored as float32)."""
    c = dict(cloud)
    s, q = c.pop("scales").astype(np.float64), c.pop("rotations").astype(np.float64)
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                   2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                   2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    M = Rm * s[:, None, :]
    Sg = M @ M.transpose(0, 2, 1)
    c["cov3D_precomp"] = np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).astype(np.float32)
    return c


def _hold(grads, o_grads, what):
    errs = compare_grads({k: v.detach().cpu().numpy() for k, v in grads.items()}, o_grads)
    print(what, errs)
    for k, e in errs.items():
        assert e <= GRAD_BOUND, (what, k, e, errs)
    return errs


# 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_plain_training_call_stores_neither_and_changes_no_gradient(monkeypatch, P):
    """SH colours + scales / rotations through GaussianRasterizer: the native call is told that neither is wanted and returns None for both;
    every gradient the caller does get is, in deterministic mode, the same bits as the low-level call that asks for all eight."""
    cam, cloud, cot = _case(P)
    all_eight = dict(zip(EIGHT, _low_level(cloud, cam, cot, DEG, "default")))
    assert all(v is not None for v in all_eight.values())              # the default: as before
    g, want, res = _autograd(cloud, cam, cot, DEG, set(cloud), monkeypatch, deterministic_backward=True)
    assert tuple(want) == (False, False)
    assert res[1] is None and res[4] is None and all(v is not None for i, v in enumerate(res) if i not in (1, 4))
    for k in ("means2D", "opacities", "means3D", "sh", "scales", "rotations"):
        assert torch.equal(g[k].reshape(all_eight[k].shape), all_eight[k]), k


# 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("binding", ["default", "ctypes"])
@pytest.mark.parametrize("want", [(False, False), (True, False), (False, True)])
def test_low_level_call_honours_want_in_both_bindings(binding, want):
    cam, cloud, cot = _case(130)
    all_eight = _low_level(cloud, cam, cot, DEG, binding)
    got = _low_level(cloud, cam, cot, DEG, binding, want=want)
    for i, (a, b) in enumerate(zip(all_eight, got)):
        if (i == 1 and not want[0]) or (i == 4 and not want[1]):
            assert b is None, EIGHT[i]
        else:
            assert torch.equal(a, b), EIGHT[i]


# 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wanted_colour_and_covariance_gradients_match_the_oracle(oracle, monkeypatch):
    """colors_precomp requiring a gradient: dL_dcolors is the output (and required without SH colours, wanted or not); cov3D_precomp requiring
    one: dL_dcov3D is, while the SH call's dL_dcolors stays unstored."""
    cam, cloud, cot = _case(130)
    pc = S.make_cloud(130, W, H, sh_degree=None, seed=3, scale_mult=25.0)
    o = oracle.run_scene(pc, cam, sh_degree=0, cotangent=cot)
    g, want, res = _autograd(pc, cam, cot, 0, {"colors_precomp"}, monkeypatch)
    assert tuple(want) == (True, False) and res[1] is not None and res[4] is None
    errs = _hold({"colors_precomp": g["colors_precomp"]}, o["grads"], "colors_precomp")
    assert "colors_precomp" in errs and o["grads"]["colors_precomp"].any()
    g, want, res = _autograd(pc, cam, cot, 0, set(), monkeypatch)     # no SH colours: the library needs dL_dcolors whatever the caller wants
    assert tuple(want) == (False, False) and res[1] is not None and res[4] is None

    cc = _cov3d_of(cloud)
    o = oracle.run_scene(cc, cam, sh_degree=DEG, cotangent=cot)
    g, want, res = _autograd(cc, cam, cot, DEG, {"cov3D_precomp", "shs"}, monkeypatch)
    assert tuple(want) == (False, True) and res[1] is None and res[4] is not None
    errs = _hold({"cov3Ds_precomp": g["cov3Ds_precomp"], "sh": g["sh"]}, o["grads"], "cov3D_precomp")
    assert "cov3Ds_precomp" in errs and o["grads"]["cov3Ds_precomp"].any()
    g, want, res = _autograd(cc, cam, cot, DEG, {"shs"}, monkeypatch)   # a precomputed covariance: dL_dcov3D stays required
    assert tuple(want) == (False, False) and res[4] is not None
