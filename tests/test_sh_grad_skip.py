"""dL_dsh is zeroed under the per-tile backward pass (csrc/render_bwd.hip: bwd_fill_zero, every wave one contiguous share as its last act) and
the per-Gaussian kernel stores only the rows whose dL_dRGB is non-zero (csrc/preprocess_bwd.hip: BwdParams::dsh_zeroed; csrc/api.hip:
backward_impl decides both halves in one call).  The read-only counter "sh_grad_skip_calls" tells which backward calls took the path.

Every GPU case runs after a NaN-filled block the size of dL_dsh has been allocated and freed, so the gradient tensor lands on memory that
held NaN: a float no wave zeroed shows up as a NaN.  Everything is held to the CPU oracle with the suite's bound (1e-3 max-rel-err per
tensor); where the oracle's dL_dsh is exactly zero the device's must be exactly zero too.

Shapes, the smallest at which the two halves can go wrong: 64x48 (12 waves) around the 64-Gaussian block edge of the per-Gaussian kernel; one
wave that fills everything (16x16, P = 1000: 12 000 float4s); more waves than there is to fill (272x16, P = 5: 17 waves, 60 float4s); the
generic layout with a tail that is no whole float4 (P = 1 at degree 2: 27 floats); a frame whose Gaussians all lie in one corner, so that
most waves return early and still have to fill.  Each oracle result is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":   # run as a program (the deterministic case starts it with another build of the library): no conftest sets the paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "wild-gaussians_amd"), os.path.join(_root, "tests")]

import wg_scenes as S
from wg_testlib import compare_grads, make_settings, to_dev

GRAD_BOUND = 1e-3   # tests/test_backward_row.py, tests/test_parity_gpu.py, tests/test_record_clear_forward.py
W0, H0, DEG = 64, 48, 3
MAIN_P = [1, 63, 64, 65, 130]
NEAR = 5            # opaque Gaussians in front of the image centre
_cache = {}


def layered_cloud(P, W=W0, H=H0, seed=11):
    """A few near, large, opaque Gaussians over the image centre (rows 0 .. NEAR-1); behind them, by row % 4: 0 a small one hidden behind the
    near ones (visible, nothing reaches it), 1 a small one off to the side (visible, reached), 2 one far outside the frame (culled), 3 one
    behind the camera (culled).  Rows 63 and 64 are of kinds 3 and 0."""
    rng = np.random.default_rng(seed)
    fx = 0.5 * W / np.tan(np.radians(60.0) * 0.5)   # wg_scenes.make_camera's focal length in pixels
    means, scales, opac = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 1))
    for i in range(P):
        kind = i % 4
        if i < NEAR:
            z, px, py, sigma, o = 1.0 + 0.1 * i, rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 15.0, 0.99
        elif kind == 0:
            z, px, py, sigma, o = rng.uniform(5.0, 8.0), rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0), 0.6, 0.8
        elif kind == 1:
            z, sigma, o = rng.uniform(4.0, 8.0), 1.5, 0.7
            px, py = rng.choice([-1.0, 1.0]) * rng.uniform(20.0, 29.0), rng.choice([-1.0, 1.0]) * rng.uniform(14.0, 21.0)
        elif kind == 2:
            z, px, py, sigma, o = rng.uniform(2.0, 6.0), 40.0 * W, rng.uniform(-5.0, 5.0), 1.5, 0.7
        else:
            z, px, py, sigma, o = -rng.uniform(1.0, 4.0), rng.uniform(-5.0, 5.0), rng.uniform(-5.0, 5.0), 1.5, 0.7
        means[i] = (px * z / fx, py * z / fx, z)
        scales[i] = sigma * abs(z) / fx * np.exp(rng.normal(0.0, 0.1, size=3))
        opac[i] = o
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    M = (DEG + 1) ** 2
    sh = rng.normal(0.0, 0.1, size=(P, M, 3))
    sh[:, 0, :] = rng.normal(0.0, 0.5, size=(P, 3))
    out = dict(means3D=means, scales=scales, rotations=q, opacities=opac, shs=sh)
    return {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in out.items()}


def corner_cloud(P=40, W=96, H=64, seed=12):
    """Every Gaussian inside the top-left 16x16 tile of a 6x4-tile frame: 23 of the 24 waves walk nothing."""
    rng = np.random.default_rng(seed)
    c = S.make_cloud(P, W, H, sh_degree=DEG, seed=seed, scale_mult=1.0)
    fx = 0.5 * W / np.tan(np.radians(60.0) * 0.5)
    z = c["means3D"][:, 2]
    c["means3D"][:, 0] = (rng.uniform(3.0, 12.0, size=P) - W / 2) * z / fx
    c["means3D"][:, 1] = (rng.uniform(3.0, 12.0, size=P) - H / 2) * z / fx
    c["scales"][:] = (0.4 * z / fx)[:, None]
    return c


def _scene(oracle, key):
    """(cam, cloud, cot, degree, oracle result): made once per key, never changed."""
    if key not in _cache:
        kind = key[0]
        deg = DEG
        if kind == "main":
            W, H, cloud = W0, H0, layered_cloud(key[1])
        elif kind == "one_wave":
            W, H = 16, 16
            cloud = S.make_cloud(1000, W, H, sh_degree=DEG, seed=3, scale_mult=4.0)
        elif kind == "many_waves":
            W, H = 272, 16
            cloud = S.make_cloud(5, W, H, sh_degree=DEG, seed=3, scale_mult=25.0)
        elif kind == "tail":
            W, H, deg = W0, H0, 2
            cloud = S.make_cloud(1, W, H, sh_degree=2, seed=3, scale_mult=25.0)
        elif kind == "corner":
            W, H, cloud = 96, 64, corner_cloud()
        elif kind == "offscreen":
            W, H = W0, H0
            cloud = S.make_cloud(70, W, H, sh_degree=DEG, seed=3, scale_mult=4.0)
            cloud["means3D"][:, 0] += 60.0 * cloud["means3D"][:, 2]
        elif kind == "precomp":
            W, H, deg = W0, H0, 0
            cloud = S.make_cloud(130, W, H, sh_degree=None, seed=3, scale_mult=25.0)
        elif kind == "clamped":
            W, H = W0, H0
            cloud = S.make_cloud(3, W, H, sh_degree=DEG, seed=3, scale_mult=25.0)
            cloud["shs"][0, 0, 0] = -6.0    # red of Gaussian 0 is negative before the clamp whatever the higher degrees add (|rest| << 1)
        else:
            raise KeyError(key)
        cam, cot = S.make_camera(W, H), S.make_cotangent(W, H)
        if kind == "clamped":
            cot[1:] = 0.0                    # dL/dpixel in red alone
        _cache[key] = (cam, cloud, cot, deg, oracle.run_scene(cloud, cam, sh_degree=deg, cotangent=cot))
    return _cache[key]


def _skip_calls():
    from diff_gaussian_rasterization import _C
    return _C.get_option("sh_grad_skip_calls")


NAMES = (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("shs", "sh"), ("colors_precomp", "colors_precomp"),
         ("scales", "scales"), ("rotations", "rotations"))


def _poison_allocator(cloud):
    """NaN-filled blocks the size of dL_dsh (several: the caching allocator may hold other free blocks of that size) and of the [P, 3]
    gradient tensors, handed back to the allocator: what the backward call allocates next starts out as NaN."""
    P = cloud["means3D"].shape[0]
    n = int(np.prod(cloud["shs"].shape)) if "shs" in cloud else 16 * P
    blocks = [torch.full((m,), float("nan"), dtype=torch.float32, device="cuda") for m in (n, n, n, n, 3 * P, 3 * P)]
    torch.cuda.synchronize()
    del blocks


def _inputs(cloud, no_grad=()):
    t = {k: to_dev(v).requires_grad_(k not in no_grad) for k, v in cloud.items()}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
    return t


def _render(rs, t, **kw):
    from diff_gaussian_rasterization import GaussianRasterizer
    return GaussianRasterizer(rs)(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t.get("shs"),
                                  colors_precomp=t.get("colors_precomp"), scales=t["scales"], rotations=t["rotations"], **kw)


def _step(cam, cloud, cot, deg, no_grad=(), **kw):
    """One forward + backward over poisoned memory -> (gradients as numpy, calls that took the path)."""
    rs = make_settings(cam, deg)
    t = _inputs(cloud, no_grad)
    color = _render(rs, t, **kw)[0]
    c0 = _skip_calls()
    _poison_allocator(cloud)
    color.backward(to_dev(cot))
    torch.cuda.synchronize()
    return {out: t[k].grad.detach().cpu().numpy() for k, out in NAMES if k in t and t[k].grad is not None}, _skip_calls() - c0


def _hold(grads, o_grads, what):
    """Finite everywhere; dL_dsh exactly zero wherever the oracle's row is exactly zero; every tensor within the bound."""
    for k, v in grads.items():
        assert np.isfinite(v).all(), (what, k)
    if "sh" in grads:
        zero_rows = (o_grads["sh"].reshape(grads["sh"].shape) == 0).all(axis=(1, 2))
        assert (grads["sh"][zero_rows] == 0).all(), (what, "rows the oracle leaves at zero")
    errs = compare_grads(grads, o_grads)
    print(what, errs)
    assert errs, what
    for k, e in errs.items():
        assert e <= GRAD_BOUND, (what, k, e, errs)


def _row_kinds(o):
    """Per Gaussian, from the oracle alone: 'c' culled, 'z' visible with an all-zero dL_dsh row, 'n' a non-zero row."""
    nz = (o["grads"]["sh"].reshape(len(o["radii"]), -1) != 0).any(axis=1)
    assert not (nz & (o["radii"] <= 0)).any()
    return np.where(o["radii"] <= 0, "c", np.where(nz, "n", "z"))


# host ---------------------------------------------------------------------------------------------------------------------------------
def test_the_main_scene_mixes_culled_untouched_and_touched_rows(oracle):
    """From the oracle alone, before anything runs on a device: a scene without the mix would let every GPU case below pass vacuously."""
    for P in MAIN_P:
        kinds = _row_kinds(_scene(oracle, ("main", P))[4])
        if P >= 63:
            assert {"c", "z", "n"} <= set(kinds), (P, "".join(kinds))
        else:
            assert "n" in kinds
    kinds = _row_kinds(_scene(oracle, ("main", 130))[4])
    assert kinds[63] != kinds[64], "".join(kinds)


# main scene ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", MAIN_P)
def test_main_scene_matches_the_oracle_over_nan_memory(oracle, P):
    cam, cloud, cot, deg, o = _scene(oracle, ("main", P))
    kinds = _row_kinds(o)
    if P >= 63:
        assert {"c", "z", "n"} <= set(kinds)
    g, took = _step(cam, cloud, cot, deg)
    assert took == 1
    _hold(g, o["grads"], f"main P={P}")


# share arithmetic of the fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", [("one_wave",), ("many_waves",), ("tail",), ("corner",)], ids=lambda k: k[0])
def test_every_float_is_filled_whatever_the_shares(oracle, key):
    """One wave for 12 000 float4s; 17 waves for 60; 27 floats (six float4s and three single floats, generic layout); waves that walk nothing."""
    cam, cloud, cot, deg, o = _scene(oracle, key)
    if key[0] == "corner":
        assert o["num_rendered"] > 0 and (o["radii"] > 0).any()
        ctx_n = o["ctx"].get("n_contrib").reshape(cam["height"], cam["width"])
        assert (ctx_n[:, 16:] == 0).all() and (ctx_n[16:, :] == 0).all(), "only the first tile may hold anything"
    g, took = _step(cam, cloud, cot, deg)
    assert took == 1
    _hold(g, o["grads"], key[0])


# paths that must not take it ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_rendered_writes_every_row_as_before(oracle):
    cam, cloud, cot, deg, o = _scene(oracle, ("offscreen",))
    assert o["num_rendered"] == 0
    g, took = _step(cam, cloud, cot, deg)
    assert took == 0
    for k, v in g.items():
        assert np.isfinite(v).all() and (v == 0).all(), k


@pytest.mark.gpu
def test_shs_without_grad_still_takes_it_and_precomputed_colours_do_not(oracle):
    """`shs` that require no gradient: the native call cannot tell -- with SH colours `dL_dsh` is a required pointer and both bindings
    always pass a tensor -- so the call TAKES the path (the counter says so: a known deviation from "only when dL_dsh is wanted",
    recorded in DESIGN.md) and every gradient that is wanted is the oracle's.  Precomputed colours have no dL_dsh and do not take it."""
    cam, cloud, cot, deg, o = _scene(oracle, ("main", 130))
    g, took = _step(cam, cloud, cot, deg, no_grad=("shs",))
    assert took == 1
    assert "sh" not in g
    _hold(g, {k: v for k, v in o["grads"].items() if k != "sh"}, "shs without grad")
    cam, cloud, cot, deg, o = _scene(oracle, ("precomp",))
    g, took = _step(cam, cloud, cot, deg)
    assert took == 0
    _hold(g, o["grads"], "precomputed colours")


# deterministic mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deterministic_mode_takes_the_path_and_repeats_bit_for_bit(oracle):
    cam, cloud, cot, deg, o = _scene(oracle, ("main", 130))
    a, took_a = _step(cam, cloud, cot, deg, deterministic_backward=True)
    b, took_b = _step(cam, cloud, cot, deg, deterministic_backward=True)
    assert (took_a, took_b) == (1, 1)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    _hold(a, o["grads"], "deterministic")
    # the old path with nothing rendered (no per-tile launch to fill under): the same zeros, compared numerically (-0.0 == +0.0)
    cam0, cloud0, cot0, deg0, _ = _scene(oracle, ("offscreen",))
    z, took = _step(cam0, cloud0, cot0, deg0, deterministic_backward=True)
    assert took == 0
    for k, v in z.items():
        assert (v == np.zeros_like(v)).all(), k
    # ... and, where a -DWG_SH_GRAD_SKIP=0 build of the library exists, the old path on THIS scene: a fresh process loads it
    # (WG_RASTERIZER_LIB), runs the same deterministic step and every tensor compares equal (numeric ==: only a zero's sign may differ)
    old_lib = _old_path_library()
    if old_lib is None:
        print("no WG_SH_GRAD_SKIP=0 build of the library: old path compared on the nothing-rendered frame only")
        return
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "old.npz")
        env = dict(os.environ, WG_RASTERIZER_LIB=old_lib)
        env.pop("WG_BINDING", None)   # (a variant library is served by the ctypes binding)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        old = dict(np.load(out))
    assert int(old.pop("took")) <= 0, "the variant library took the path: not a -DWG_SH_GRAD_SKIP=0 build"   # (-1: a build without the counter)
    assert set(old) == set(a)
    for k in a:
        assert np.isfinite(old[k]).all() and (a[k] == old[k]).all(), k
    print("old path (variant library) == this build on", sorted(a))


def _old_path_library():
    """A build of the library with -DWG_SH_GRAD_SKIP=0, if there is one: named by WG_SH_GRAD_SKIP_OFF_LIB, or where
    `WG_BUILD_VARIANT=sh_grad_skip_off WG_EXTRA_FLAGS=-DWG_SH_GRAD_SKIP=0 python wild-gaussians_amd/build.py` puts it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.environ.get("WG_SH_GRAD_SKIP_OFF_LIB"), os.path.join(root, "wild-gaussians_amd", "build", "sh_grad_skip_off", "libwg_rasterizer.so")):
        if p and os.path.exists(p):
            return p
    return None


# a pointer that is not 16-byte aligned -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unaligned_dL_dsh_is_filled_from_its_first_float_to_its_last(oracle, monkeypatch):
    """torch's allocations are 512-byte aligned, so the fill's single-float head never runs through the bindings as they are.  Here the ctypes
    binding's allocation of dL_dsh is replaced by a NaN-filled tensor that starts 4 bytes into its block: three floats in front of the
    aligned body, 779 float4s, one float behind them (P = 65: 3120 floats), and the per-Gaussian kernel in its generic layout (the
    coalesced ones need the alignment), whose per-row guard and dropped zero loop for culled rows are held on the way."""
    from diff_gaussian_rasterization import _C
    cam, cloud, cot, deg, o = _scene(oracle, ("main", 65))
    P, M = cloud["shs"].shape[:2]
    real_empty = torch.empty
    made = []

    def empty(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if shape != (P, M, 3):
            return real_empty(*size, **kw)
        block = torch.full((P * M * 3 + 1,), float("nan"), dtype=torch.float32, device=kw.get("device", "cuda"))
        made.append(block)
        return block[1:].view(P, M, 3)
    prev = _C.use_binding("ctypes")
    try:
        monkeypatch.setattr(torch, "empty", empty)
        g, took = _step(cam, cloud, cot, deg)
    finally:
        monkeypatch.undo()
        _C.use_binding(prev)
    assert took == 1 and len(made) == 1
    assert made[0].data_ptr() % 16 == 0 and torch.isnan(made[0][0]).item(), "the float in front of the tensor is not the call's to write"
    assert np.isfinite(made[0][1:].cpu().numpy()).all()
    _hold(g, o["grads"], "unaligned dL_dsh")


# clamped channels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_row_whose_only_channel_is_clamped_stays_zero(oracle):
    cam, cloud, cot, deg, o = _scene(oracle, ("clamped",))
    assert o["radii"][0] > 0 and (o["grads"]["sh"][0] == 0).all() and (o["grads"]["sh"][1:] != 0).any()
    assert (o["grads"]["means3D"][0] != 0).any(), "the Gaussian is blended: its mean has a gradient"
    g, took = _step(cam, cloud, cot, deg)
    assert took == 1
    assert (g["sh"][0] == 0).all()
    _hold(g, o["grads"], "clamped red")
    _hold({"means3D": g["means3D"][:1]}, {"means3D": o["grads"]["means3D"][:1]}, "clamped red, its own dL_dmean3D")


# retained graph -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_second_backward_over_a_retained_graph_fills_and_stores_again(oracle):
    cam, cloud, cot, deg, o = _scene(oracle, ("main", 130))
    rs = make_settings(cam, deg)
    t = _inputs(cloud)
    keys = list(t)
    color = _render(rs, t)[0]
    c0 = _skip_calls()
    _poison_allocator(cloud)
    first = torch.autograd.grad(color, [t[k] for k in keys], to_dev(cot), retain_graph=True)
    _poison_allocator(cloud)
    second = torch.autograd.grad(color, [t[k] for k in keys], to_dev(cot))
    assert _skip_calls() - c0 == 2
    names = dict(NAMES)
    a = {names[k]: v.cpu().numpy() for k, v in zip(keys, first)}
    b = {names[k]: v.cpu().numpy() for k, v in zip(keys, second)}
    _hold(a, o["grads"], "first backward")
    _hold(b, o["grads"], "second backward")
    _hold(b, a, "second against first")   # (tests/test_record_clear_forward.py's bound for the same pair: float atomics)


if __name__ == "__main__":   # <out.npz>: the main scene's deterministic step with whichever library WG_RASTERIZER_LIB names
    _g, _took = _step(S.make_camera(W0, H0), layered_cloud(130), S.make_cotangent(W0, H0), DEG, deterministic_backward=True)
    np.savez(sys.argv[1], took=_took, **_g)
