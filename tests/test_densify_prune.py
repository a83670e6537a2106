"""Fused densify-and-prune, its exact quantile and reset_opacity (include/wg_densify_prune.h; wg_fused_gaussians.densify_and_prune / quantile /
reset_opacity; wg_integration.apply_optins(densify=True)) against GaussianModel.densify_and_prune and reset_opacity
(wildgaussians/method.py:1249-1468).

The yardstick is the float64 restatement of tests/densify_prune_lib.py, evaluated on the float32 inputs; its docstring derives the bounds
used here (u = 2^-24): Q within u (|Q| + 3 |b - a|) (exact at a tie), a child's position within 50 u sum_k |z_k| exp(s_k) + 2 u |xyz_new|, a
child's scale within 6 u + 4 u |scale|, a reset opacity within 85 u + (84 u x + u) / (1 - x) + 4 u |y|.  Decisions (the origin and kind of every
output row, the three counts, ratio) must match EXACTLY: the inputs keep every decision a relative 3e-4 away from its threshold and the
restatement asserts 1e-4.  Copied values are bit-identical to their source rows; moments and buffers of new rows are exactly 0.  The
recorded run of the reference's own methods (tests/golden/densify_caller.npz, made by tests/golden/make_densify_golden.py) falls within the
same bounds, which pins the restatement to the reference.
"""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import densify_prune_lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "densify_caller.npz")
U = L.U


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = (err / bound).max() if err.size else 0.0
    print(f"{what}: n={err.size} worst error / bound = {ratio:.3f}")
    assert np.isfinite(np.asarray(got)).all() and ratio <= 1.0, what


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_follows_method_py():
    ref = "/root/reference/wildgaussians/method.py"
    if not os.path.isfile(ref):
        pytest.skip("reference checkout not present")
    src = open(ref).read()
    for frag in ("grads = self.xyz_grad / self.denom", "grads[grads.isnan()] = 0.0", "ratio = (torch.norm(grads, dim=-1) >= max_grad).float().mean()",
                 "Q = torch.quantile(grads_abs.reshape(-1), 1 - ratio)", "torch.max(scales, dim=1).values <= self.config.percent_dense*scene_extent",
                 "torch.max(scales, dim=1).values > self.config.percent_dense*scene_extent", "samples = torch.normal(mean=means, std=stds)",
                 'new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + gaussians["xyz"][selected_pts_mask].repeat(N, 1)',
                 "new_scaling = self.scaling_inverse_activation(scales[selected_pts_mask].repeat(N,1) / (0.8*N))",
                 "prune_mask = (opacity < min_opacity).squeeze()", "big_points_ws = scales.max(dim=1).values > 0.1 * extent",
                 "return clone - before, split - clone, split - prune", "q = r / norm[:, None]",
                 "opacities_new = torch.min(current_opacity_with_filter, torch.ones_like(current_opacity_with_filter)*0.01)",
                 "scales_after_square = scales_square + torch.square(self.filter_3D)", "opacities_new = opacities_new / coef[..., None]",
                 "opacities_new = torch.special.logit(opacities_new)"):
        assert frag in src, frag


def test_input_helper_is_deterministic_and_populates_every_class():
    a, b = L.make_inputs(2048, 11), L.make_inputs(2048, 11)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["scales"], L.make_inputs(2048, 12)["scales"])
    r = L.restate(a)
    assert min(r["n_out"]) > 10 and r["pruned_originals"] > 10 and r["pruned_children"] > 2 and r["nan_stats"] > 10 and r["ties_at_Q"] > 1
    assert L.restate(L.make_inputs(2048, 11, ga_mode="continuous"))["Q_bound"] > 0


def test_restatement_holds_the_reference_methods_own_run():
    g = np.load(GOLDEN)
    d = L.make_inputs(int(g["P"]), int(g["seed"]))
    r = L.restate(d, None, g["noise"])
    assert np.array_equal(r["origin"], g["origin"]) and r["counts"] == tuple(g["counts"])
    assert r["ratio"] == float(g["ratio"]) and abs(float(g["Q"]) - r["Q"]) <= r["Q_bound"]
    assert r["n_out"][1] > 50 and r["n_out"][2] > 50 and r["pruned_children"] > 10 and r["nan_stats"] > 50 and r["ties_at_Q"] > 1
    kept = r["child_kept"]
    within(g["child_xyz"], r["child_xyz"][kept], r["child_xyz_bound"][kept], "reference child xyz vs restatement")
    within(g["child_scales"], r["child_scales"][kept], r["child_scales_bound"][kept], "reference child scales vs restatement")
    src, new = g["origin"][:, 0], g["origin"][:, 1] > 0
    for n in L.BUFFERS:   # the buffers are carried, not reset: copied for originals, zero for new rows
        assert np.array_equal(g["buf_" + n][~new], d[n][src[~new]]) and not g["buf_" + n][new].any(), n
    assert np.array_equal(g["opacities_exp_avg"][~new], d["opacities.exp_avg"][src[~new]]) and not g["opacities_exp_avg"][new].any()
    scales = d["scales"][src].copy()
    scales[g["origin"][:, 1] >= 2] = g["child_scales"]
    y, bound = L.reset_opacity64(d["opacities"][src], scales, g["buf_filter_3D"])
    within(g["reset_opacities"].reshape(-1), y, bound, "reference reset_opacity vs restatement")


def test_densify_prune_abi_exported():
    lib = C.CDLL(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so"))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wg_densify_prune.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(wg_[a-z0-9_]+)\s*\(", text))
    assert names == {"wg_densify_scratch_bytes", "wg_quantile", "wg_densify_plan", "wg_densify_apply", "wg_reset_opacity"}
    for n in names:
        getattr(lib, n)
    assert '#include "wg_densify_prune.h"' in open(os.path.join(ROOT, "include", "wg_densify.h")).read()
    import wg_fused_gaussians as FG
    assert C.sizeof(FG._DensifyCounts) == 80 and C.sizeof(FG._DensifyParams) == 24 and C.sizeof(FG._DensifyArray) == 24
    sb = FG._lib.wg_densify_scratch_bytes
    assert sb(-1) == 0 and sb(0) > 0 and sb(0) % 256 == 0 and 5 * 10 ** 6 <= sb(10 ** 6) <= 5.2 * 10 ** 6   # 5 bytes per Gaussian
    prm, cnt = FG._DensifyParams(2e-4, 0.005, 0.05, 0.5, 1, 1), FG._DensifyCounts()
    cnt.n_cloned = 7
    assert FG._lib.wg_densify_plan(-1, C.byref(prm), None, None, None, None, None, None, C.addressof(cnt), None) == -1
    assert FG._lib.wg_densify_plan(8, C.byref(prm), None, None, None, None, None, None, C.addressof(cnt), None) == -1   # null pointers, P > 0
    assert FG._lib.wg_densify_plan(0, C.byref(prm), None, None, None, None, None, None, C.addressof(cnt), None) == 0 and cnt.n_cloned == 0
    assert FG._lib.wg_densify_apply(0, C.byref(cnt), None, 0, None, None, None, None, None, None, None) == 0
    cnt.n_out[2], cnt.n_out[3] = 1, 0
    assert FG._lib.wg_densify_apply(8, C.byref(cnt), None, 0, None, None, None, None, None, None, None) == -1   # the two copies differ
    assert FG._lib.wg_densify_apply(8, C.byref(FG._DensifyCounts()), None, 49, None, None, None, None, None, None, None) == -1
    assert FG._lib.wg_quantile(0, None, 0.5, None, None, None) == -1 and FG._lib.wg_quantile(4, None, 0.5, None, None, None) == -1
    assert FG._lib.wg_reset_opacity(0, None, None, None, None, None, None, None) == 0
    assert FG._lib.wg_reset_opacity(4, None, None, None, None, None, None, None) == -1
    d = {k: torch.from_numpy(v) for k, v in L.make_inputs(16, 0).items()}
    with pytest.raises(RuntimeError, match="no CPU path"):
        FG.densify_and_prune({k: d[k] for k in ("xyz", "scales", "rotations", "opacities")}, None, {k: d[k] for k in L.BUFFERS}, **L.DEFAULTS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FG.quantile(torch.zeros(4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FG.reset_opacity(d["opacities"], d["scales"], d["filter_3D"])


class _FakeModel:
    def _setup_optimizers(self): pass
    def add_densification_stats(self, a, b): pass
    def get_gaussians(self): pass
    def compute_3D_filter(self, cameras): pass
    def densify_and_prune(self, max_grad, min_opacity, extent, enable_size_pruning, skyradius=None): pass
    def reset_opacity(self): pass


def test_densify_optin_is_off_by_default_and_undo_is_complete():
    from wg_integration import apply_optins
    fake = types.SimpleNamespace(GaussianModel=_FakeModel, ssim=lambda *a, **k: None, eval_sh=lambda *a, **k: None)
    before = dict(_FakeModel.__dict__)
    undo = apply_optins(fake)   # defaults
    assert _FakeModel.__dict__["densify_and_prune"] is before["densify_and_prune"] and _FakeModel.__dict__["reset_opacity"] is before["reset_opacity"]
    undo()
    undo = apply_optins(fake, ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False, densify=True)
    assert _FakeModel.__dict__["densify_and_prune"] is not before["densify_and_prune"]
    assert _FakeModel.__dict__["reset_opacity"] is not before["reset_opacity"]
    assert _FakeModel.__dict__["compute_3D_filter"] is before["compute_3D_filter"]
    undo()
    assert dict(_FakeModel.__dict__) == before


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def run_fused(d, params=None, noise=None, generator=None):
    import wg_fused_gaussians as FG
    p = dict(L.DEFAULTS, **(params or {}))
    dev = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    tensors = {k: dev[k] for k in L.PARAMS if k in dev}
    adam = {k: {"step": torch.tensor(3.0), "exp_avg": dev[k + ".exp_avg"], "exp_avg_sq": dev[k + ".exp_avg_sq"]} for k in tensors}
    stats = {k: dev[k] for k in L.BUFFERS if k in dev}
    res = FG.densify_and_prune(tensors, adam, stats, noise=None if noise is None else torch.from_numpy(noise).cuda(), generator=generator, **p)
    for k, v in dev.items():   # the inputs are left untouched
        assert np.array_equal(v.cpu().numpy(), d[k], equal_nan=True), k
    return res


def check_result(res, d, params, what):
    """Everything the issue asks of one call: decisions exact, copies bit-identical, new rows' state zero, computed values within bounds."""
    noise = res.noise.cpu().numpy()
    r = L.restate(d, params, noise)
    origin = res.origin.cpu().numpy()
    assert res.counts == r["counts"] and res.n_out == r["n_out"] and res.n_hot == r["n_hot"], (what, res.counts, r["counts"])
    assert np.array_equal(origin, r["origin"]), what
    assert res.ratio == r["ratio"]
    if r["Q"] is None:
        assert res.Q is None
    else:
        print(f"{what}: Q={res.Q!r} restated {r['Q']!r} bound {r['Q_bound']:.3e} ties at Q {r['ties_at_Q']}")
        assert abs(res.Q - r["Q"]) <= r["Q_bound"], what
    src, kind = origin[:, 0], origin[:, 1]
    child, new = kind >= 2, kind > 0
    for k, t in res.tensors.items():
        got = t.cpu().numpy()
        assert got.shape == (origin.shape[0],) + d[k].shape[1:] and got.dtype == np.float32
        same = ~child if k in ("xyz", "scales") else np.ones_like(child)
        assert np.array_equal(got[same], d[k][src[same]]), (what, k)
        m, v = (x.cpu().numpy() for x in res.adam_state[k])
        assert np.array_equal(m[~new], d[k + ".exp_avg"][src[~new]]) and np.array_equal(v[~new], d[k + ".exp_avg_sq"][src[~new]]), (what, k)
        assert not m[new].any() and not v[new].any(), (what, k)
    for k, t in res.stats.items():
        got = t.cpu().numpy()
        assert got.shape == (origin.shape[0],) + d[k].shape[1:]
        assert np.array_equal(got[~new], d[k][src[~new]], equal_nan=True) and not got[new].any(), (what, k)
    if child.any():
        kept = r["child_kept"]
        within(res.tensors["xyz"].cpu().numpy()[child], r["child_xyz"][kept], r["child_xyz_bound"][kept], what + ": child xyz")
        within(res.tensors["scales"].cpu().numpy()[child], r["child_scales"][kept], r["child_scales_bound"][kept], what + ": child scales")
    return r


@pytest.mark.gpu
def test_fused_on_the_fixture_against_the_restatement_and_the_reference_run():
    g = np.load(GOLDEN)
    d = L.make_inputs(int(g["P"]), int(g["seed"]))
    res = run_fused(d, None, g["noise"])
    r = check_result(res, d, None, "fixture")
    assert np.array_equal(res.origin.cpu().numpy(), g["origin"]) and res.counts == tuple(g["counts"])
    assert res.ratio == float(g["ratio"]) and abs(res.Q - float(g["Q"])) <= 2 * r["Q_bound"]
    child, kept = g["origin"][:, 1] >= 2, r["child_kept"]
    for k, b in (("xyz", "child_xyz_bound"), ("scales", "child_scales_bound")):   # both sides' bounds added
        diff = np.abs(res.tensors[k].cpu().numpy()[child].astype(np.float64) - g["child_" + k])
        assert (diff <= 2 * r[b][kept]).all(), k
    for n in L.BUFFERS:
        assert np.array_equal(res.stats[n].cpu().numpy(), g["buf_" + n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("P,ga_mode,sh_degree,n_embed,params", [
    (1, "grid", 1, 6, None), (2, "continuous", 0, 0, None), (255, "grid", 1, 6, None), (4097, "continuous", 3, 24, None),
    (100001, "continuous", 3, 24, None), (100001, "grid", 1, 6, None), (30000, "continuous", 2, 0, dict(use_abs_gradient=False)),
    (30000, "grid", 1, 6, dict(enable_size_pruning=False)), (30000, "continuous", 1, 6, dict(extent=2.0, max_grad=0.0004))])
def test_fused_against_the_restatement(P, ga_mode, sh_degree, n_embed, params):
    d = L.make_inputs(P, 100 + P % 97 + sh_degree, sh_degree=sh_degree, n_embed=n_embed, ga_mode=ga_mode, params=params)
    if not (params or {}).get("use_abs_gradient", True):
        d = {k: v for k, v in d.items() if not k.startswith("xyz_gradient_accum_abs")}
    gen = torch.Generator(device="cuda").manual_seed(P)
    check_result(run_fused(d, params, generator=gen), d, params, f"P={P} {ga_mode} sh={sh_degree} {params}")


@pytest.mark.gpu
def test_many_zeros_in_ga_and_an_integer_rank():
    """(a) 90 % of the Gaussians were never seen (statistics 0 / 0 -> NaN -> 0), every seen one is hot by g (ratio ~ 0.1) and half of the seen ones
    have ga = 0 too: 95 % of ga is zero, the rank 0.9 (n - 1) falls among the zeros, Q = 0 exactly and EVERY Gaussian satisfies ga >= Q -- all
    are cloned or split, as in the reference.  (b) nobody reaches max_grad: ratio = 0, q = 1, the rank is n - 1 with w = 0 and Q is the largest
    ga; only its holders are hot."""
    d = L.make_inputs(20000, 5, ga_mode="continuous")
    rng = np.random.default_rng(0)
    unseen = rng.uniform(size=(20000, 1)) < 0.9
    for k in ("denom", "xyz_grad", "xyz_gradient_accum_abs"):
        d[k] = np.where(unseen, np.float32(0), d[k])
    d["xyz_gradient_accum_abs"] = np.where(rng.uniform(size=(20000, 1)) < 0.5, np.float32(0), d["xyz_gradient_accum_abs"])
    p = dict(max_grad=1e-9)
    res = run_fused(d, p)
    r = check_result(res, d, p, "many zeros")
    assert 0.05 < res.ratio < 0.15 and res.Q == 0.0 and r["q_stats"]["a"] == 0.0 and res.counts[0] + res.counts[1] == 20000
    d = L.make_inputs(20000, 6, ga_mode="continuous")
    p = dict(max_grad=1.0)
    res = run_fused(d, p)
    r = check_result(res, d, p, "integer rank")
    assert res.ratio == 0.0 and r["q_stats"]["w"] == 0.0 and r["q_stats"]["lo"] == 19999 and res.counts[0] + res.counts[1] == 1
    with np.errstate(invalid="ignore", divide="ignore"):
        assert res.Q == float(np.nanmax(d["xyz_gradient_accum_abs"] / d["denom"]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 1000, 1025, (1 << 20) + 3])
def test_quantile_against_torch_quantile(n):
    import wg_fused_gaussians as FG
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(np.float32)        # both signs
    v[rng.uniform(size=n) < 0.3] = 0.0                    # many ties
    x = torch.from_numpy(v)
    for q in (0.0, 1.0, 0.5, 0.25, 0.123, 0.9371, 1.0 - 2.0 ** -12):   # 0.25 and 0.5 give w = 0 at n = 1025
        got = float(FG.quantile(x.cuda(), q))
        s = L.quantile64(v, q)
        ref = float(torch.quantile(x, q))
        print(f"n={n} q={q}: got {got!r} torch {ref!r} restated {s['Q']!r} w={s['w']}")
        assert abs(got - s["Q"]) <= s["bound"] and abs(got - ref) <= 2 * s["bound"], (n, q)
    assert L.quantile64(np.zeros(1025, np.float32), 0.25)["w"] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(1 << 24) + 1, 40_000_003])
def test_quantile_beyond_torchs_limit(n):
    """torch.quantile refuses more than 2^24 elements; the selection returns, and equals a float64 selection on the host."""
    import wg_fused_gaussians as FG
    v = np.random.default_rng(n).standard_normal(n, dtype=np.float32)
    np.abs(v, out=v)
    x = torch.from_numpy(v).cuda()
    for q in (0.9, 0.5 + 2.0 ** -30):
        got = float(FG.quantile(x, q))
        s = L.quantile64(v, q)
        print(f"n={n} q={q}: got {got!r} restated {s['Q']!r} lo={s['lo']} w={s['w']}")
        assert abs(got - s["Q"]) <= U * abs(s["Q"]), (n, q)   # float64 arithmetic, one rounding to float32


@pytest.mark.gpu
def test_reset_opacity_against_float64():
    import wg_fused_gaussians as FG
    d = L.make_inputs(50001, 3)
    o, s, f = (torch.from_numpy(d[k]).cuda() for k in ("opacities", "scales", "filter_3D"))
    m, v = torch.from_numpy(d["opacities.exp_avg"]).cuda(), torch.from_numpy(d["opacities.exp_avg_sq"]).cuda()
    got = FG.reset_opacity(o, s, f, m, v)
    y, bound = L.reset_opacity64(d["opacities"], d["scales"], d["filter_3D"])
    assert got.shape == o.shape and np.array_equal(o.cpu().numpy(), d["opacities"])
    within(got.cpu().numpy().reshape(-1), y, bound, "reset_opacity")
    assert not m.any() and not v.any()


class _Model(torch.nn.Module):
    """The parts of the caller's GaussianModel the two swapped methods touch, built the way the caller builds them."""

    def __init__(self, d, fused_adam):
        super().__init__()
        import wg_fused_gaussians as FG
        self.config = types.SimpleNamespace(percent_dense=L.DEFAULTS["percent_dense"], use_gof_abs_gradient=True)
        self._dynamically_sized_props = ["xyz", "features_dc", "features_rest", "scales", "rotations", "opacities", "xyz_grad", "denom", "filter_3D",
                                         "embeddings", "max_radii2D", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max"]
        for k in L.PARAMS:
            self.register_parameter(k, torch.nn.Parameter(torch.from_numpy(d[k]).cuda()))
        for k in L.BUFFERS:
            self.register_buffer(k, torch.from_numpy(d[k]).cuda())
        self.register_parameter("appearance_embeddings", torch.nn.Parameter(torch.randn(5, 8, device="cuda")))
        # lr = 0: the steps build the moments and leave the parameters (and with them every decision's distance to its threshold) alone
        groups = [{"params": [getattr(self, k)], "lr": 0.0, "name": k} for k in L.PARAMS] + \
                 [{"params": [self.appearance_embeddings], "lr": 1e-3, "name": "appearance_embeddings"}]
        self.optimizer = (FG.FusedAdam if fused_adam else torch.optim.Adam)(groups, lr=1.0, eps=1e-15)

    def densify_and_prune(self, *a, **k):
        raise AssertionError("the original must not run")

    def reset_opacity(self):
        raise AssertionError("the original must not run")

    def backward_and_step(self):
        loss = sum((getattr(self, k) ** 2).sum() for k in L.PARAMS) + (self.appearance_embeddings ** 2).sum()
        loss.backward()
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fused_adam", [True, False])
def test_optin_end_to_end(fused_adam):
    from wg_integration import apply_optins
    d = L.make_inputs(6000, 21)
    fake = types.SimpleNamespace(GaussianModel=_Model)
    model = _Model(d, fused_adam)
    model.backward_and_step()   # the moments exist and are non-zero
    before = {k: getattr(model, k).detach().cpu().numpy() for k in L.PARAMS}
    mom = {k: model.optimizer.state[getattr(model, k)]["exp_avg"].cpu().numpy() for k in L.PARAMS}
    shared = model.optimizer.state[model.appearance_embeddings]["exp_avg"].clone()
    assert all(np.array_equal(before[k], d[k]) for k in L.PARAMS)
    r = L.restate(d)
    undo = apply_optins(fake, ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False, densify=True)
    try:
        counts = model.densify_and_prune(L.DEFAULTS["max_grad"], L.DEFAULTS["min_opacity"], L.DEFAULTS["extent"], True, skyradius=None)
        assert counts == r["counts"]
        n_new, src, new = r["origin"].shape[0], r["origin"][:, 0], r["origin"][:, 1] > 0
        params, buffers = dict(model.named_parameters()), dict(model.named_buffers())
        assert len(model.optimizer.state) == len(L.PARAMS) + 1
        for g in model.optimizer.param_groups:
            k, p = g["name"], g["params"][0]
            if k == "appearance_embeddings":   # not per-Gaussian: untouched
                assert p is model.appearance_embeddings and torch.equal(model.optimizer.state[p]["exp_avg"], shared)
                continue
            assert p is params[k] is getattr(model, k) and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.shape[0] == n_new
            st = model.optimizer.state[p]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 1.0
            assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape
            m = st["exp_avg"].cpu().numpy()
            assert np.array_equal(m[~new], mom[k][src[~new]]) and not m[new].any()
            if k not in ("xyz", "scales"):
                assert np.array_equal(p.detach().cpu().numpy(), before[k][src])
        for k in L.BUFFERS:
            assert buffers[k] is getattr(model, k) and buffers[k].shape == (n_new,) + d[k].shape[1:]
        model.backward_and_step()   # the optimizer steps the new parameters with the moved state
        for g in model.optimizer.param_groups:
            st = model.optimizer.state[g["params"][0]]
            assert len(model.optimizer.state) == len(L.PARAMS) + 1 and st["exp_avg"].shape == g["params"][0].shape
            assert float(st["step"]) == 2.0 and bool(st["exp_avg"].abs().sum() > 0)
        old = model.opacities
        y, bound = L.reset_opacity64(old.detach().cpu().numpy(), model.scales.detach().cpu().numpy(), model.filter_3D.cpu().numpy())
        model.reset_opacity()
        p = model.opacities
        assert p is not old and p is model.optimizer.param_groups[L.PARAMS.index("opacities")]["params"][0] and old not in model.optimizer.state
        st = model.optimizer.state[p]
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 2.0
        within(p.detach().cpu().numpy().reshape(-1), y, bound, "opt-in reset_opacity")
        model.backward_and_step()
    finally:
        undo()
    with pytest.raises(AssertionError, match="original"):
        model.densify_and_prune(0.0002, 0.005, 5.0, True)
    with pytest.raises(AssertionError, match="original"):
        model.reset_opacity()


@pytest.mark.gpu
def test_refused_inside_a_stream_capture_and_noise_is_checked():
    import wg_fused_gaussians as FG
    d = L.make_inputs(512, 1)
    with pytest.raises(RuntimeError, match="noise must be"):
        run_fused(d, None, np.zeros((3, 3), np.float32))
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True   # the binding's own check; the library refuses a capturing stream the same way
    try:
        with pytest.raises(RuntimeError, match="stream capture"):
            run_fused(d)
    finally:
        torch.cuda.is_current_stream_capturing = real
    assert FG.densify_and_prune is not None
