"""The gradient record of a frame that expects an atomic-mode backward call is zeroed by the frame's own forward render launch
(csrc/render_fwd.hip: fwd_clear_record, every wave's last act; csrc/api.hip: ForwardFrame::clear_floats, take_record_clean): the backward call that
finds the frame's mark hands the ordering launch nothing to clear.  Read-only counters tell which path ran: "record_clean_frames" (forward calls
whose render launch cleared) and "record_clean_calls" (backward calls that cleared nothing).

Gradients are held to the CPU oracle with the bound tests/test_backward_row.py uses (1e-3 max-rel-err per tensor).  The shapes are the smallest
at which the clear can go wrong: 64x48 (12 waves) around the 64-Gaussian block edge, one wave that clears everything (16x16, P = 1000), more waves
than float4s to clear (272x16, P = 5: 17 waves, 15 float4s) and the two-colour call's thirteen floats per Gaussian (P = 3: 39 floats, rounded
up to 40).  Each oracle result is computed once and shared."""
import numpy as np
import pytest
import torch

import wg_scenes as S
from wg_testlib import compare_grads, make_settings, to_dev

GRAD_BOUND = 1e-3   # tests/test_backward_row.py, tests/test_parity_gpu.py: gradients <= 1e-3 max-rel-err per tensor
DEG = 3
SHAPES = [(64, 48, 1), (64, 48, 63), (64, 48, 64), (64, 48, 65), (64, 48, 130), (16, 16, 1000), (272, 16, 5)]
_oracle_cache = {}


def _case(oracle, W, H, P):
    """(cam, cloud, cot, oracle result) of a shape: made once, never changed."""
    key = (W, H, P)
    if key not in _oracle_cache:
        cam, cot = S.make_camera(W, H), S.make_cotangent(W, H)
        cloud = S.make_cloud(P, W, H, sh_degree=DEG, seed=3, scale_mult=25.0 if P < 1000 else 4.0)
        _oracle_cache[key] = (cam, cloud, cot, oracle.run_scene(cloud, cam, sh_degree=DEG, cotangent=cot))
    return _oracle_cache[key]


def _counters():
    from diff_gaussian_rasterization import _C
    return _C.get_option("record_clean_frames"), _C.get_option("record_clean_calls")


def _inputs(cloud, grad=True):
    t = {k: to_dev(v).requires_grad_(grad) for k, v in cloud.items()}
    t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=grad)
    return t


def _render(rs, t, **kw):
    from diff_gaussian_rasterization import GaussianRasterizer
    return GaussianRasterizer(rs)(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t.get("shs"),
                                  colors_precomp=t.get("colors_precomp"), scales=t["scales"], rotations=t["rotations"], **kw)


NAMES = (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("shs", "sh"), ("colors_precomp", "colors_precomp"),
         ("scales", "scales"), ("rotations", "rotations"))


def _grads_of(t):
    return {out: t[k].grad.detach().cpu().numpy() for k, out in NAMES if k in t and t[k].grad is not None}


def _hold(grads, o_grads, what):
    errs = compare_grads(grads, o_grads)
    print(what, errs)
    assert errs, what
    for k, e in errs.items():
        assert e <= GRAD_BOUND, (what, k, e, errs)


def _poison_allocator(nbytes):
    """A block of the caching allocator the size of the frame's geometry buffer, filled with NaN and handed back: the next allocation of that
    size -- the geometry buffer, gradient record inside -- starts out as NaN."""
    blk = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device="cuda")
    blk.fill_(float("nan"))
    del blk


def _geometry_bytes(cloud, cam):
    from wg_testlib import run_hip_native
    return run_hip_native(cloud, cam, sh_degree=DEG)["buffers"][0].numel()


# 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H,P", SHAPES)
def test_gradients_over_a_forward_cleared_record_match_the_oracle(oracle, W, H, P):
    """The frame's render launch clears, its backward call clears nothing, the gradients are the oracle's -- over a geometry buffer that
    held NaN before the forward call, so a float4 that no wave zeroed shows up as a NaN gradient."""
    cam, cloud, cot, o = _case(oracle, W, H, P)
    rs = make_settings(cam, DEG)
    nbytes = _geometry_bytes(cloud, cam)
    t = _inputs(cloud)
    f0, b0 = _counters()
    _poison_allocator(nbytes)
    color, radii, _ = _render(rs, t)
    f1, b1 = _counters()
    color.backward(to_dev(cot))
    f2, b2 = _counters()
    assert (f1 - f0, b1 - b0, f2 - f1, b2 - b1) == (1, 0, 0, 1)
    assert (radii.cpu().numpy() == o["radii"]).all()
    g = _grads_of(t)
    for k, v in g.items():
        assert np.isfinite(v).all(), k
    _hold(g, o["grads"], f"{W}x{H} P={P}")


# 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_colour_call_clears_thirteen_floats_per_gaussian(oracle):
    """P = 3 with a second colour set: 39 floats of record, cleared as ten float4s.  Each colour set's gradient is the oracle's for that set
    alone; the geometry gradients are those of both losses, i.e. the sum of the two oracle runs."""
    W, H, P = 64, 48, 3
    cam, cot1, cot2 = S.make_camera(W, H), S.make_cotangent(W, H, seed=1), S.make_cotangent(W, H, seed=2)
    cloud = S.make_cloud(P, W, H, sh_degree=None, seed=3, scale_mult=25.0)
    colors2 = np.random.default_rng(5).uniform(0, 1, size=(P, 3)).astype(np.float32)
    o1 = oracle.run_scene(cloud, cam, sh_degree=0, cotangent=cot1)
    o2 = oracle.run_scene(dict(cloud, colors_precomp=colors2), cam, sh_degree=0, cotangent=cot2)
    assert (o1["radii"] > 0).any()
    rs = make_settings(cam, 0)
    from wg_testlib import run_hip_native
    nbytes = run_hip_native(cloud, cam, sh_degree=0)["buffers"][0].numel()
    t = _inputs(cloud)
    c2 = to_dev(colors2).requires_grad_(True)
    f0, b0 = _counters()
    _poison_allocator(nbytes)
    img1, radii, _, img2 = _render(rs, t, colors_precomp2=c2)
    ((img1 * to_dev(cot1)).sum() + (img2 * to_dev(cot2)).sum()).backward()
    f1, b1 = _counters()
    assert (f1 - f0, b1 - b0) == (1, 1)
    g = _grads_of(t)
    both = {k: o1["grads"][k] + o2["grads"][k] for k in ("means3D", "means2D", "opacities", "scales", "rotations")}
    both["colors_precomp"] = o1["grads"]["colors_precomp"]
    _hold(g, both, "two colours, first set and geometry")
    _hold({"colors_precomp": c2.grad.cpu().numpy()}, {"colors_precomp": o2["grads"]["colors_precomp"]}, "two colours, second set")


# 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_second_backward_over_a_retained_graph_clears_for_itself(oracle):
    """The mark is taken once: the second backward call over the frame finds a record the first one accumulated into, clears it as ever
    and gives the same gradients (within the bound: float atomics)."""
    cam, cloud, cot, o = _case(oracle, 64, 48, 130)
    rs = make_settings(cam, DEG)
    t = _inputs(cloud)
    keys = [k for k in t]
    color, _, _ = _render(rs, t)
    f0, b0 = _counters()
    first = torch.autograd.grad(color, [t[k] for k in keys], to_dev(cot), retain_graph=True)
    f1, b1 = _counters()
    second = torch.autograd.grad(color, [t[k] for k in keys], to_dev(cot))
    f2, b2 = _counters()
    assert (b1 - b0, b2 - b1, f2 - f0) == (1, 0, 0)
    names = dict(NAMES)
    a = {names[k]: v.cpu().numpy() for k, v in zip(keys, first)}
    b = {names[k]: v.cpu().numpy() for k, v in zip(keys, second)}
    _hold(a, o["grads"], "first backward")
    _hold(b, o["grads"], "second backward")
    _hold(b, a, "second against first")


# 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frames_that_do_not_take_the_path_are_unchanged(oracle):
    """deterministic_backward frames (the ordered sum writes every record in full), a forward under torch.no_grad() and the colour-only
    backward: neither counter moves where the path must not be taken, and the outputs are the same bits whatever the buffers held before."""
    from diff_gaussian_rasterization import _C
    cam, cloud, cot, o = _case(oracle, 64, 48, 130)
    rs = make_settings(cam, DEG)
    nbytes = _geometry_bytes(cloud, cam)

    def det_step(poison):
        t = _inputs(cloud)
        if poison:
            _poison_allocator(nbytes)
        color, _, _ = _render(rs, t, deterministic_backward=True)
        color.backward(to_dev(cot))
        return color.detach().cpu().numpy(), _grads_of(t)
    f0, b0 = _counters()
    img_a, ga = det_step(False)
    img_b, gb = det_step(True)
    assert _counters() == (f0, b0)                         # deterministic frames: no clear in the forward launch, no mark to take
    assert np.array_equal(img_a, img_b)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    _hold(ga, o["grads"], "deterministic")

    with torch.no_grad():                                  # no backward call expected: the render launch does not clear
        img_c = _render(rs, _inputs(cloud, grad=False))[0].cpu().numpy()
    assert _counters() == (f0, b0)
    assert np.array_equal(img_c, img_a)

    # colour-only backward: nothing is recorded, so the frame's mark is not taken
    pc = S.make_cloud(130, 64, 48, sh_degree=None, seed=3, scale_mult=25.0)
    oc = oracle.run_scene(pc, cam, sh_degree=0, cotangent=cot)
    rs0 = make_settings(cam, 0)
    tc = _inputs(pc, grad=False)
    tc["colors_precomp"].requires_grad_(True)
    img_d = _render(rs0, tc, colour_gradients_only=True)[0]
    b1 = _counters()[1]
    img_d.backward(to_dev(cot))
    assert _counters()[1] == b1
    with torch.no_grad():
        img_e = _render(rs0, _inputs(pc, grad=False))[0]
    assert torch.equal(img_d.detach(), img_e)
    _hold({"colors_precomp": tc["colors_precomp"].grad.cpu().numpy()}, {"colors_precomp": oc["grads"]["colors_precomp"]}, "colour-only")
    assert _C.get_option("record_clean_calls") == b1
