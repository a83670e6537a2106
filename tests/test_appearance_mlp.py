"""The fused appearance MLP (include/wg_appearance_mlp.h, wg_fused_gaussians.appearance_mlp / embedding_forward, the `appearance_mlp`
opt-in) against the float64 oracle of tests/appearance_mlp_lib.py.  The gate everywhere is |kernel - float64| <= the oracle's a-priori
float32 rounding bound, element by element: no tuned tolerance, no excluded elements.

GPU shapes are the smallest at which the kernel can still go wrong: a row tile is 64 rows walked as two halves of 32, so P = 1, 63, 64, 65
and 5 tiles + 37 with max_workgroups = 3 give idle workgroups, a ragged half, a ragged tile, workgroups with two tiles and one with a
ragged last tile; widths 6 / 5 are no multiple of the MFMA's K.  The automatic grid is reached once, at 2 tiles per workgroup + 37 rows,
with the weight gradients under a sparse cotangent (at that size the dense bound would let a lost tile pass)."""
import ctypes as C
import functools
import inspect
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import appearance_mlp_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wg_appearance_mlp.h")
WNAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]


def FG():
    import wg_fused_gaussians
    return wg_fused_gaussians


@functools.lru_cache(maxsize=None)
def case(P, G, E, seed):
    return L.make_case(P, G, E, seed)


@functools.lru_cache(maxsize=None)
def dense_oracle(P, G, E, seed):
    c = case(P, G, E, seed)
    cot = L.dense_cotangent(P, seed)
    return c, cot, L.oracle(c, cot)


# ---- CPU: the C-ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_names_are_exported_and_nothing_else():
    names = set(re.findall(r"\b(wg_appearance_mlp_\w+)\s*\(", open(HEADER).read()))
    assert names == {"wg_appearance_mlp_scratch_floats", "wg_appearance_mlp_forward", "wg_appearance_mlp_backward"}
    lib = FG()._lib._name
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("wg_appearance_mlp")}
    assert exported == names


def test_scratch_size_arithmetic():
    fg = FG()
    f = fg._lib.wg_appearance_mlp_scratch_floats
    assert fg.MLP_PARTIAL_FLOATS == 128 * 64 + 128 * 128 + 6 * 128 + 128 + 128 + 8
    macros = dict(re.findall(r"#define (WG_MLP_\w+) +(\d+)\b", open(HEADER).read()))
    assert int(macros["WG_MLP_TILE_ROWS"]) == fg.MLP_TILE_ROWS and int(macros["WG_MLP_SCRATCH_HEAD_FLOATS"]) == fg.MLP_SCRATCH_HEAD_FLOATS
    for P in (0, 1, 63, 64, 65, 128, 129, 1000, 3_000_000):
        for wgs in (1, 3, 7, 256):
            tiles = (P + 63) // 64
            assert f(P, wgs) == fg.MLP_SCRATCH_HEAD_FLOATS + min(tiles, wgs) * fg.MLP_PARTIAL_FLOATS, (P, wgs)
    assert f(0, 0) == fg.MLP_SCRATCH_HEAD_FLOATS   # no tile: no device is asked
    assert f(-1, 3) < 0 and f(10, -1) < 0


def _valid_args(fg, P=65, widths=(3, 24), E=32, wgs=3, wgrad=True):
    """A well-formed argument block over FAKE device addresses: every call made with it must be refused before any device work."""
    a = fg._MlpArgs()
    fake = 0x10000
    a.struct_size = C.sizeof(fg._MlpArgs)
    a.P = P
    a.num_segments = len(widths)
    for i, w in enumerate(widths):
        a.segments[i].ptr, a.segments[i].width, a.segments[i].row_stride = fake, w, w + 5
        a.grad_segment[i], a.grad_row_stride[i] = fake, w
    a.shared_width, a.shared = E, (fake if E else None)
    a.W1 = a.b1 = a.W2 = a.b2 = a.W3 = a.b3 = fake
    a.out_scale, a.max_workgroups = 0.01, wgs
    a.out = a.dL_dout = fake
    a.grad_shared = fake if E else None
    if wgrad:
        a.dW1 = a.db1 = a.dW2 = a.db2 = a.dW3 = a.db3 = fake
    a.scratch = fake
    a.scratch_floats = fg._lib.wg_appearance_mlp_scratch_floats(P, wgs)
    return a


MALFORMED = {
    "struct_size short": lambda a: setattr(a, "struct_size", a.struct_size - 8),
    "P negative": lambda a: setattr(a, "P", -1),
    "no segments": lambda a: setattr(a, "num_segments", 0),
    "four segments": lambda a: setattr(a, "num_segments", 4),
    "null segment": lambda a: setattr(a.segments[1], "ptr", None),
    "width 0": lambda a: setattr(a.segments[0], "width", 0),
    "widths sum 65": lambda a: (setattr(a.segments[1], "width", 62), setattr(a.segments[1], "row_stride", 62)),
    "row_stride < width": lambda a: setattr(a.segments[1], "row_stride", 23),
    "shared_width 65": lambda a: setattr(a, "shared_width", 65),
    "shared_width negative": lambda a: setattr(a, "shared_width", -1),
    "shared null with a width": lambda a: setattr(a, "shared", None),
    "null W1": lambda a: setattr(a, "W1", None),
    "null b2": lambda a: setattr(a, "b2", None),
    "null W3": lambda a: setattr(a, "W3", None),
    "max_workgroups negative": lambda a: setattr(a, "max_workgroups", -2),
}
MALFORMED_FWD = {"null out": lambda a: setattr(a, "out", None)}
MALFORMED_BWD = {
    "null dL_dout": lambda a: setattr(a, "dL_dout", None),
    "five weight gradients": lambda a: setattr(a, "db2", None),
    "one weight gradient": lambda a: [setattr(a, n, None) for n in WNAMES[1:]],
    "grad stride < width": lambda a: a.grad_row_stride.__setitem__(1, 23),
    "null scratch": lambda a: setattr(a, "scratch", None),
    "scratch one float short": lambda a: setattr(a, "scratch_floats", a.scratch_floats - 1),
    "scratch sized for fewer workgroups": lambda a: setattr(a, "max_workgroups", 7),   # P = 200: 4 tiles, sized for 3 workgroups
}


@pytest.mark.parametrize("which", sorted(MALFORMED) + sorted(MALFORMED_FWD))
def test_malformed_forward_refused_before_device_work(which):
    fg = FG()
    a = _valid_args(fg)
    {**MALFORMED, **MALFORMED_FWD}[which](a)
    assert fg._lib.wg_appearance_mlp_forward(C.byref(a)) == -1   # WG_ERR_INVALID_ARGUMENT; a launch on these addresses would be WG_ERR_HIP or a fault


@pytest.mark.parametrize("which", sorted(MALFORMED) + sorted(MALFORMED_BWD))
def test_malformed_backward_refused_before_device_work(which):
    fg = FG()
    a = _valid_args(fg, P=200)
    {**MALFORMED, **MALFORMED_BWD}[which](a)
    assert fg._lib.wg_appearance_mlp_backward(C.byref(a)) == -1


def test_null_argument_block_refused():
    fg = FG()
    assert fg._lib.wg_appearance_mlp_forward(None) == -1 and fg._lib.wg_appearance_mlp_backward(None) == -1


# ---- CPU: the opt-in ---------------------------------------------------------------------------------------------------------------------
def _fake_method_module(**kw):
    class EmbeddingModel(L.StubEmbedding):
        pass
    return types.SimpleNamespace(GaussianModel=type("GaussianModel", (), {}), EmbeddingModel=EmbeddingModel), EmbeddingModel


OFF = dict(ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False)


def test_optin_is_off_by_default_and_sits_before_uncertainty_metrics():
    import wg_integration
    params = inspect.signature(wg_integration.apply_optins).parameters
    assert params["appearance_mlp"].default is False
    names = list(params)
    assert names.index("appearance_mlp") == names.index("uncertainty_metrics") - 1 and names[-1] == "uncertainty_metrics"
    mod, EM = _fake_method_module()
    before = EM.__dict__.get("forward", None)
    undo = wg_integration.apply_optins(mod, **OFF)
    assert EM.__dict__.get("forward", None) is before
    undo()


def test_optin_swaps_and_undoes():
    import wg_integration
    mod, EM = _fake_method_module()
    orig = EM.forward
    undo = wg_integration.apply_optins(mod, appearance_mlp=True, **OFF)
    assert EM.forward is not orig
    undo()
    assert EM.forward is orig


@pytest.mark.parametrize("why", ["cpu", "float64", "appearance_model_sh", "hidden 64", "out 96", "not sequential"])
def test_optin_forwards_uncovered_calls_to_the_original(why):
    import wg_integration
    mod, EM = _fake_method_module()
    undo = wg_integration.apply_optins(mod, appearance_mlp=True, **OFF)
    try:
        kw = {"hidden 64": dict(hidden=64), "out 96": dict(out=96), "appearance_model_sh": dict(sh=True)}.get(why, {})
        m = EM(3 + 24 + 32, **kw)
        if why == "not sequential":
            m.mlp = torch.nn.Linear(59, 6)
        dt = torch.float64 if why == "float64" else torch.float32
        m = m.to(dt)
        g, a, c = torch.zeros(4, 24, dtype=dt), torch.zeros(4, 32, dtype=dt), torch.zeros(4, 48, dtype=dt)
        assert m(g, a, c) == "original"
        assert len(m.calls) == 1 and m.calls[0][0] is g and m.calls[0][1] is a and m.calls[0][2] is c
        assert m(g, a, c, viewdir="v") == "original" and m.calls[1][3] == "v"
    finally:
        undo()


# ---- CPU: the oracle ---------------------------------------------------------------------------------------------------------------------
ALL_CASES = [(P, G, E, 100 + i) for i, (P, G, E) in enumerate((P, G, E) for G, E in ((24, 32), (6, 5)) for P in (1, 63, 64, 65, 357))]


def test_robust_row_cap():
    for P, G, E, seed in ALL_CASES + list(L.GOLDEN_CASES):
        c = case(P, G, E, seed)
        assert c["discarded"] < L.MAX_DISCARD, (P, G, E, seed, c["discarded"])
        f = L.forward64(L.case_x64(c), [w.double() for w in c["weights"]])
        assert bool(((f["z1"].abs() > 2 * f["e1"]) & (f["z2"].abs() > 2 * f["e2"])).all())
        if P >= 63:   # the mask is exercised: a good share of the units is off, and a good share on
            assert 0.2 < float(f["m1"].double().mean()) < 0.8 and 0.2 < float(f["m2"].double().mean()) < 0.8


def _golden():
    z = np.load(L.GOLDEN)
    assert [tuple(x) for x in json.loads(str(z["cases"]))] == [tuple(x) for x in L.GOLDEN_CASES]
    return z


def _module_truth(i):
    P, G, E, seed = L.GOLDEN_CASES[i]
    c = case(P, G, E, seed)
    return c, L.module_oracle(c, L.golden_cot48(P, seed))


ORACLE_KEY = {"toned": "toned", "d_features": "d_features", "d_gemb": "d_gemb", "d_aemb": "d_aemb_rows"}


@pytest.mark.parametrize("i", range(len(L.GOLDEN_CASES)))
def test_oracle_is_pinned_to_the_reference_fixture(i):
    z = _golden()
    c, r = _module_truth(i)
    for k in L.GOLDEN_KEYS:
        ok = ORACLE_KEY.get(k, k)
        want64 = torch.from_numpy(z[f"{k}64_{i}"])
        assert want64.dtype == torch.float64 and want64.shape == r[ok].shape
        assert float(((r[ok] - want64).abs() / want64.abs().clamp_min(1.0)).max()) <= 1e-12, k   # the oracle restates the reference
        got32 = torch.from_numpy(z[f"{k}32_{i}"])
        assert got32.dtype == torch.float32
        assert L.ratio(got32, r[ok], r["e_" + ok]) <= 1.0, k                                      # and PyTorch's float32 is within the bound


def test_oracle_against_the_reference_class():
    checkout = os.environ.get("WG_REFERENCE_CHECKOUT", "/root/reference")
    if not os.path.exists(os.path.join(checkout, "wildgaussians", "method.py")):
        pytest.skip("no checkout of the reference on this machine")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_appearance_mlp_golden", os.path.join(ROOT, "tests", "golden", "make_appearance_mlp_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    cls = mk.reference_class(checkout)
    c = case(65, 24, 32, 999)
    r = L.module_oracle(c, L.golden_cot48(65, 999))
    for dtype, gate in ((torch.float64, None), (torch.float32, 1.0)):
        res = L.run_module(cls.forward, mk.reference_model(cls, c, dtype), c, True, dtype)
        for k in L.GOLDEN_KEYS:
            ok = ORACLE_KEY.get(k, k)
            got = torch.from_numpy(res[k])
            if gate is None:
                assert float(((r[ok] - got).abs() / got.abs().clamp_min(1.0)).max()) <= 1e-12, k
            else:
                assert L.ratio(got, r[ok], r["e_" + ok]) <= gate, k


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _run(c, cot, per_row, colour_view, max_workgroups, need=("inputs", "shared", "weights")):
    """appearance_mlp forward + backward on the device -> dict with out, dx (colour | gemb [| aemb rows]), dshared, dW1..db3."""
    fg = FG()
    dev = "cuda"
    feats = c["features"].to(dev)
    colour = (feats[:, :3] if colour_view else feats[:, :3].contiguous()).detach().requires_grad_("inputs" in need)
    gemb = c["gemb"].to(dev).requires_grad_("inputs" in need)
    W = [w.to(dev).requires_grad_("weights" in need) for w in c["weights"]]
    if per_row:
        aemb = c["aemb"][None].repeat(c["P"], 1).to(dev).requires_grad_("inputs" in need)
        out = fg.appearance_mlp((colour, gemb, aemb), W, max_workgroups=max_workgroups)
    else:
        aemb = c["aemb"].to(dev).requires_grad_("shared" in need)
        out = fg.appearance_mlp((colour, gemb), W, shared=aemb, max_workgroups=max_workgroups)
    assert out.shape == (c["P"], 6) and out.dtype == torch.float32
    out.backward(cot.to(dev))
    r = {"out": out.detach()}
    if "inputs" in need:
        parts = [colour.grad, gemb.grad] + ([aemb.grad] if per_row else [])
        r["dx"] = torch.cat(parts, 1)
    else:
        assert colour.grad is None and gemb.grad is None
    if not per_row:
        r["dshared"] = aemb.grad
    elif "inputs" in need:
        r["dshared"] = aemb.grad.sum(0)   # not gated: only the shared path's own result is
    for n, w in zip(WNAMES, W):
        r[n] = w.grad
    return r


def _assert_within(r, o, keys, per_row, tag=""):
    Kr = r["dx"].shape[1] if "dx" in r else None
    for k in keys:
        want, bound = o[k], o["e_" + k]
        if k == "dx":
            want, bound = want[:, :Kr], bound[:, :Kr]
        q = L.ratio(r[k], want, bound)
        print(f"{tag} {k}: max err/bound {q:.3f}")
        assert q <= 1.0, (tag, k, q)


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [True, False], ids=["aemb-per-row", "aemb-shared"])
@pytest.mark.parametrize("P,G,E,seed", ALL_CASES, ids=[f"P{c[0]}-G{c[1]}-E{c[2]}" for c in ALL_CASES])
def test_forward_backward_within_bound(P, G, E, seed, per_row):
    c, cot, o = dense_oracle(P, G, E, seed)
    for colour_view in (True, False):
        r = _run(c, cot, per_row, colour_view, max_workgroups=3)
        keys = ["out", "dx"] + WNAMES + ([] if per_row else ["dshared"])
        _assert_within(r, o, keys, per_row, tag=f"P={P} G={G} E={E} {'row' if per_row else 'shared'} view={colour_view}")


@pytest.mark.gpu
def test_automatic_grid():
    fg = FG()
    wgs = (fg.appearance_mlp_scratch_floats(10 ** 9, 0) - fg.MLP_SCRATCH_HEAD_FLOATS) // fg.MLP_PARTIAL_FLOATS
    assert wgs >= 1
    P, G, E, seed = 2 * 64 * wgs + 37, 24, 32, 4242
    c = case(P, G, E, seed)
    assert c["discarded"] < L.MAX_DISCARD
    cot = L.dense_cotangent(P, seed)
    o = L.oracle(c, cot)
    r = _run(c, cot, False, True, 0, need=("inputs", "shared"))
    _assert_within(r, o, ["out", "dx"], False, tag=f"auto grid {wgs} workgroups, P={P}, dense")
    # the issue's sparse cotangent (one row of every 64-row block, the first row and the last), and the same per 32-row half tile, which
    # is the unit this kernel could lose: n is a few hundred to ~1000, and one lost row is far over the bound
    for block, per_row in ((64, False), (32, True)):
        cot = L.sparse_cotangent(P, seed, block=block)
        o = L.oracle(c, cot)
        r = _run(c, cot, per_row, True, 0)
        _assert_within(r, o, ["out", "dx"] + WNAMES + ([] if per_row else ["dshared"]), per_row, tag=f"auto grid, sparse/{block}, per_row={per_row}")
        # the yardstick sees a lost row: dropping one non-zero row from the float64 sum moves some weight gradient past its bound
        row = int((cot != 0).any(1).nonzero()[3])
        cot2 = cot.clone()
        cot2[row] = 0
        o2 = L.oracle(c, cot2)
        lost = max(L.ratio(o2[k], o[k], o["e_" + k]) for k in WNAMES)
        print(f"a lost row under the sparse/{block} cotangent: {lost:.1f} x the bound")
        assert lost > (10.0 if block == 64 else 4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [True, False], ids=["aemb-per-row", "aemb-shared"])
def test_two_calls_give_the_same_bits(per_row):
    P, G, E, seed = ALL_CASES[4]
    c, cot, o = dense_oracle(P, G, E, seed)
    a = _run(c, cot, per_row, True, 3)
    b = _run(c, cot, per_row, True, 3)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    a0 = _run(c, cot, per_row, True, 0)
    b0 = _run(c, cot, per_row, True, 0)
    for k in a0:
        assert torch.equal(a0[k], b0[k]), k


@pytest.mark.gpu
def test_per_row_and_shared_agree_with_one_oracle():
    P, G, E, seed = ALL_CASES[4]
    c, cot, o = dense_oracle(P, G, E, seed)
    row = _run(c, cot, True, True, 3)
    sh = _run(c, cot, False, True, 3)
    _assert_within(row, o, ["out", "dx"] + WNAMES, True, tag="per-row")
    _assert_within(sh, o, ["out", "dx", "dshared"] + WNAMES, False, tag="shared")
    assert L.ratio(sh["dshared"], o["dshared"], o["e_dshared"]) <= 1.0   # dL_dshared within the bound of the row sum


@pytest.mark.gpu
def test_dead_unit_gets_exact_zeros():
    P, G, E, seed = ALL_CASES[3]
    c = dict(case(P, G, E, seed))
    u = 37
    W = [w.clone() for w in c["weights"]]
    W[0][u] = 0
    W[1][u] = 0
    c["weights"] = W
    cot = L.dense_cotangent(P, seed)
    for per_row in (True, False):
        r = _run(c, cot, per_row, True, 3)
        assert bool((r["dW1"][u] == 0).all()) and float(r["db1"][u]) == 0.0 and bool((r["dW2"][:, u] == 0).all())
        assert bool((r["dW1"] != 0).any()) and bool((r["dW2"] != 0).any())


def _raw_backward(c, cot, grad_ptrs, grad_strides, grad_shared, max_workgroups=3):
    fg = FG()
    dev = "cuda"
    feats, gemb, aemb = c["features"].to(dev), c["gemb"].to(dev), c["aemb"].to(dev)
    W = [w.to(dev) for w in c["weights"]]
    g = cot.to(dev).contiguous()
    a = fg._MlpArgs()
    fg._mlp_fill(a, [feats[:, :3], gemb], aemb, W, 0.01, max_workgroups, torch.cuda.current_stream().cuda_stream)
    a.dL_dout = g.data_ptr()
    for i, (p, s) in enumerate(zip(grad_ptrs, grad_strides)):
        a.grad_segment[i], a.grad_row_stride[i] = p, s
    a.grad_shared = grad_shared
    n = fg.appearance_mlp_scratch_floats(c["P"], max_workgroups)
    scratch = torch.empty(n, device=dev)
    a.scratch, a.scratch_floats = scratch.data_ptr(), n
    assert fg._lib.wg_appearance_mlp_backward(C.byref(a)) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_null_gradient_pointer_leaves_its_buffer_untouched():
    P, G, E, seed = ALL_CASES[4]
    c, cot, o = dense_oracle(P, G, E, seed)
    sentinel = -12345.0
    # one [P, 3 + G] buffer: the colour's gradient goes to its first three columns (row stride 3 + G), gembedding's pointer is NULL
    buf = torch.full((P, 3 + G), sentinel, device="cuda")
    gsh = torch.full((E + 8,), sentinel, device="cuda")
    _raw_backward(c, cot, [buf.data_ptr(), None], [3 + G, 0], gsh.data_ptr())
    assert bool((buf[:, 3:] == sentinel).all()) and bool((gsh[E:] == sentinel).all())
    assert L.ratio(buf[:, :3], o["dx"][:, :3], o["e_dx"][:, :3]) <= 1.0
    assert L.ratio(gsh[:E], o["dshared"], o["e_dshared"]) <= 1.0
    # no segment wants a gradient, only the shared embedding does
    buf.fill_(sentinel)
    gsh.fill_(sentinel)
    _raw_backward(c, cot, [None, None], [0, 0], gsh.data_ptr())
    assert bool((buf == sentinel).all()) and bool((gsh[E:] == sentinel).all())
    assert L.ratio(gsh[:E], o["dshared"], o["e_dshared"]) <= 1.0


@pytest.mark.gpu
def test_optimize_embedding_pattern():
    """Only the shared embedding requires a gradient (WildGaussians.optimize_embedding): it is correct, and nothing else gets one."""
    P, G, E, seed = ALL_CASES[4]
    c, cot, o = dense_oracle(P, G, E, seed)
    r = _run(c, cot, False, True, 3, need=("shared",))
    assert all(r[n] is None for n in WNAMES)
    _assert_within(r, o, ["out", "dshared"], False, tag="embedding only")


@pytest.mark.gpu
def test_empty_input():
    fg = FG()
    c = case(1, 24, 32, ALL_CASES[0][3])
    W = [w.cuda().requires_grad_(True) for w in c["weights"]]
    aemb = c["aemb"].cuda().requires_grad_(True)
    out = fg.appearance_mlp((torch.zeros(0, 3, device="cuda"), torch.zeros(0, 24, device="cuda")), W, shared=aemb, max_workgroups=3)
    assert out.shape == (0, 6)
    for w in W:
        w.grad = torch.full_like(w, 7.0)
    out.backward(torch.zeros(0, 6, device="cuda"))
    # autograd ADDS to an existing .grad: the kernel's own result is the difference, all zeros
    assert all(bool((w.grad == 7.0).all()) for w in W) and bool((aemb.grad == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["aemb-per-row", "aemb-shared"])
@pytest.mark.parametrize("i", range(len(L.GOLDEN_CASES)))
def test_embedding_forward_against_the_fixture(i, shared):
    fg = FG()
    z = _golden()
    c, r = _module_truth(i)
    m = L.load_weights(L.StubEmbedding(c["K"]), c["weights"], torch.float32, "cuda")
    res = L.run_module(lambda mod, g, a, col: fg.embedding_forward(mod, g, a, col, max_workgroups=3), m, c, not shared, torch.float32, "cuda")
    assert m.calls == []   # the fused path ran, not the module's own forward
    for k in L.GOLDEN_KEYS:
        ok = ORACLE_KEY.get(k, k)
        want, bound = torch.from_numpy(z[f"{k}64_{i}"]), r["e_" + ok]
        if k == "d_aemb" and shared:
            want, bound = want.sum(0), r["e_dshared"]
        got = torch.from_numpy(res[k])
        assert got.shape == want.shape, k
        q = L.ratio(got, want, bound)
        print(f"case {i} shared={shared} {k}: max err/bound {q:.3f}")
        assert q <= 1.0, (k, q)


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["float64", "appearance_model_sh", "hidden 64"])
def test_uncovered_device_calls_reach_the_original(why):
    fg = FG()
    kw = {"hidden 64": dict(hidden=64), "appearance_model_sh": dict(sh=True)}.get(why, {})
    dt = torch.float64 if why == "float64" else torch.float32
    m = L.StubEmbedding(59, **kw).to(device="cuda", dtype=dt)
    g, a, c = torch.zeros(4, 24, dtype=dt, device="cuda"), torch.zeros(4, 32, dtype=dt, device="cuda"), torch.zeros(4, 48, dtype=dt, device="cuda")
    assert fg.embedding_forward(m, g, a, c) == "original" and m.calls[0][0] is g
