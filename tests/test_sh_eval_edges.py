"""Fused eval_sh (include/wg_sh_eval.h, csrc/sh_eval.hip) held element by element to a float64 oracle within a-priori rounding bounds
(tests/sh_eval_lib.py) at the wave, alignment and degree edges of its four kernels.

CPU: the oracle is pinned to the reference function's recorded outputs, a float32 emulation of the kernels' arithmetic is accepted by
the checker in both orders of rounding, and seeded mutants of that emulation are rejected.  GPU: the C-ABI between guard regions, at
every dispatch path; the wrapper's call shapes.  No element of any output is left out of any comparison."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sh_eval_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the checker itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [3, 1])
def test_oracle_reproduces_the_reference_functions_recorded_outputs(deg):
    """tests/golden/sh_eval_caller.npz holds the reference's own eval_sh in float32 inside its caller's chain (normalize, clamp_max,
    + 0.5, clamp_min; tests/golden/make_sh_eval_caller_golden.py).  The oracle runs that chain in float64 on the same seeded inputs.

    Tolerances, per element, from the bound b of sh_eval_lib.bounds (the reference's float32 expression has the same chains of roundings
    as the kernel's) plus the fixture's own float32 rounding:
      the direction: `normalize` in float32 rounds each component by at most 4 u relative (three squares and two sums under a square
        root, the root, the division); a polynomial of degree <= 3 moves by at most 3 * 4 u of its absolute-monomial value for that,
        so b grows by 12 u of the same sum: b * (1 + 12 / roundings of b);
      colour: one more rounding, of `+ 0.5`: u |colour|;
      positions: the direction's gradient g goes through the Jacobian of normalize, (g - d (d.g)) / |v|.  The reference's autograd sums
        a direction component's gradient over more paths than the kernel's 16-rounding chain -- 40 is allowed for it (the limit
        sh_eval_lib keeps R under), 12 for the rounded direction as above, 12 for the float32 arithmetic of normalize's own backward:
        64 u (G_i + |d_i| sum_j |d_j| G_j) / |v| with G the absolute-monomial value of the derivative polynomial.
    The clamp at 0 is a decision; the fixture's rows all stand further from it than the tolerance (asserted), so nothing is left out."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sh_eval_caller.npz"))
    g = torch.Generator().manual_seed(9)
    P = 20000
    feats, xyz, cot = torch.randn(P, 48, generator=g), torch.randn(P, 3, generator=g), torch.randn(P, 3, generator=g)
    rows = gold[f"colour_deg{deg}"].shape[0]
    feats, xyz, cot = feats[:rows].numpy(), xyz[:rows].numpy(), cot[:rows].numpy()
    n = L.n_coefficients(deg)
    v = (xyz - np.array([0.3, -0.2, 4.0], np.float32)).astype(np.float64)   # the caller's float32 subtraction
    length = np.linalg.norm(v, axis=1, keepdims=True)
    d = v / length
    d32 = d.astype(np.float32)
    sh = np.ascontiguousarray(np.minimum(feats, np.float32(1.0)).reshape(rows, 16, 3).transpose(0, 2, 1))
    zero_cot = np.zeros_like(cot)
    pre = L.oracle(deg, sh, d32, zero_cot)["out"] + 0.5
    b_out = L.bounds(deg, sh, d32, zero_cot)["out"] * (1 + 12 / (n + 8)) + L.U * np.abs(pre)
    assert (np.abs(pre) > b_out).all()   # no row sits on the clamp's threshold
    assert (np.abs(np.maximum(pre, 0.0) - gold[f"colour_deg{deg}"]) <= b_out).all()
    cot_in = np.where(pre > 0, cot, np.float32(0)).astype(np.float32)   # clamp_min's backward
    ref, b = L.oracle(deg, sh, d32, cot_in), L.bounds(deg, sh, d32, cot_in)
    to_leaf = lambda t: t.transpose(0, 2, 1).reshape(rows, 48)
    grad_feats = to_leaf(ref["grad_sh"]) * (feats <= 1.0)   # clamp_max's backward
    assert (np.abs(grad_feats - gold[f"grad_coefficients_deg{deg}"]) <= to_leaf(b["grad_sh"]) * (1 + 12 / 8)).all()
    assert not gold[f"grad_coefficients_deg{deg}"].reshape(rows, 16, 3)[:, n:].any()
    gd = ref["grad_dirs"]
    grad_xyz = (gd - d * (d * gd).sum(axis=1, keepdims=True)) / length
    G = b["grad_dirs"] / (L.GRAD_DIRS_ROUNDINGS * L.U)
    b_xyz = 64 * L.U * (G + np.abs(d) * (np.abs(d) * G).sum(axis=1, keepdims=True)) / length
    assert (np.abs(grad_xyz - gold[f"grad_positions_deg{deg}"]) <= b_xyz).all()


def _all_inputs():
    """(name, degree, sh, dirs, cot) of every input the GPU tests run: the mixed cases and the one-hot rows."""
    for c in L.CASES:
        yield (L.case_id(c), c.deg) + L.case_inputs(c)
    yield ("one_hot", 3) + L.one_hot_inputs()


@pytest.mark.parametrize("fused", [False, True], ids=["separate_multiply_and_add", "products_kept_in_float64"])
def test_emulated_kernel_arithmetic_is_accepted(fused):
    """The float32 emulation of the kernels' arithmetic passes the checker on every input of the GPU tests, all degrees, once with
    every product rounded before its add and once with the products kept in float64 (an FMA): the bounds are attainable."""
    worst = dict.fromkeys(L.TENSORS, 0.0)
    for name, deg, sh, dirs, cot in _all_inputs():
        got = L.emulate(deg, sh, dirs, cot, fused=fused)
        for t, r in L.check(got, deg, sh, dirs, cot).items():
            worst[t] = max(worst[t], r)
        without = L.emulate(deg, sh, dirs, cot, fused=fused, want_dirs=False)
        assert "grad_dirs" not in without and np.array_equal(without["grad_sh"].view(np.uint32), got["grad_sh"].view(np.uint32))
    print("largest error / bound:", worst)
    assert max(worst.values()) <= 1.0


# Which inputs catch which mutant (asserted below): "mixed" = at least one of sh_eval_lib.CASES, "one_hot" = the one-hot rows.
# The one-hot rows are degree 3, K = 16 and three full waves, so the three mutants that need K > N or a partial wave cannot show there;
# every arithmetic mutant is caught by both, the one-hot rows holding each basis term and each monomial on its own.
CAUGHT_BY = {
    "sign": {"mixed", "one_hot"},
    "c3_1": {"mixed", "one_hot"},
    "drop_s14": {"mixed", "one_hot"},
    "k_equals_n": {"mixed"},
    "tail_row": {"mixed"},
    "stale_grad_sh": {"mixed"},
    "swap_rows": {"mixed", "one_hot"},
}


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutants_of_the_emulation_are_rejected(mutant):
    """Each planted fault fails the checker on at least one of the GPU tests' inputs, for every seed that places it."""
    assert set(CAUGHT_BY) == set(L.MUTANTS)
    for seed in range(3):
        caught = {}
        for name, deg, sh, dirs, cot in _all_inputs():
            try:
                L.check(L.emulate(deg, sh, dirs, cot, mutant=mutant, seed=seed), deg, sh, dirs, cot)
            except AssertionError:
                caught[name] = True
        kinds = {"one_hot" if name == "one_hot" else "mixed" for name in caught}
        print(mutant, "seed", seed, "caught by", len(caught), "inputs, the one-hot rows", "among them" if "one_hot" in caught else "not")
        assert kinds == CAUGHT_BY[mutant], (mutant, seed, sorted(caught))


def test_checker_takes_nan_only_where_the_oracle_has_it():
    sh, dirs, cot = L.coefficients(8, 16, 0), L.directions(8, 0), L.cotangent(8, 0)
    sh[3, 1, 6] = np.nan
    got = L.emulate(2, sh, dirs, cot)
    L.check(got, 2, sh, dirs, cot)
    assert np.argwhere(np.isnan(got["out"])).tolist() == [[3, 1]]
    for bad in (np.nan, 0.0):   # a NaN where the oracle is finite, a number where it is NaN
        wrong = {k: v.copy() for k, v in got.items()}
        wrong["out"][(4, 1) if np.isnan(bad) else (3, 1)] = bad
        with pytest.raises(AssertionError):
            L.check(wrong, 2, sh, dirs, cot)
    wrong = {k: v.copy() for k, v in got.items()}
    wrong["grad_sh"][0, 0, 9] = 1e-30   # beyond the active degree: exactly 0 or nothing
    with pytest.raises(AssertionError):
        L.check(wrong, 2, sh, dirs, cot)


# ---- GPU: the C-ABI between guard regions --------------------------------------------------------------------------------------------
NAN_BITS = 0x7FC0BEEF   # a quiet NaN with a recognisable payload
GUARD = 64
_LIB = []


def _lib():
    if not _LIB:
        lib = C.CDLL(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so"))
        lib.wg_eval_sh_forward.restype = C.c_int
        lib.wg_eval_sh_forward.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
        lib.wg_eval_sh_backward.restype = C.c_int
        lib.wg_eval_sh_backward.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
        _LIB.append(lib)
    return _LIB[0]


class _Region:
    """`n` floats inside a larger buffer filled with a NaN bit pattern: GUARD floats before and `after` floats behind them, the region
    itself `off` floats (4 bytes each) past a 256-byte boundary."""

    def __init__(self, n, off=0, after=GUARD, values=None):
        self.n, self.start = n, GUARD + off
        self.bits = torch.full((self.start + n + after,), NAN_BITS, dtype=torch.int32, device="cuda")
        assert self.bits.data_ptr() % 256 == 0
        if values is not None:
            self.bits[self.start:self.start + n] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1).view(np.int32)).cuda()
        self.before = self.bits.clone()
        self.ptr = self.bits.data_ptr() + 4 * self.start

    def values(self):
        return self.bits[self.start:self.start + self.n].cpu().numpy().view(np.float32)

    def assert_guards_intact(self, name):
        outside = torch.cat([self.bits[:self.start], self.bits[self.start + self.n:]]).cpu().numpy().view(np.uint32)
        assert (outside == NAN_BITS).all(), f"{name}: {int((outside != NAN_BITS).sum())} guard words written"

    def assert_unchanged(self, name):
        assert torch.equal(self.bits, self.before), f"{name}: an input was written"


def _run(P, deg, K, sh, dirs, cot, misalign=None, want_dirs=True):
    """Forward and backward through the C-ABI on the null stream.  Outputs and guards start as NaN bits; `sh` and `dirs` are followed by
    64 rows of NaN.  Guards and inputs are compared as words after the calls."""
    lib = _lib()
    d_sh = _Region(P * 3 * K, off=1 if misalign == "sh" else 0, after=64 * 3 * K, values=sh)
    d_dirs = _Region(P * 3, after=64 * 3, values=dirs)
    d_cot = _Region(P * 3, values=cot)
    out, grad_sh = _Region(P * 3), _Region(P * 3 * K, off=1 if misalign == "grad_sh" else 0)
    grad_dirs = _Region(P * 3) if want_dirs else None
    assert d_sh.ptr % 16 == (4 if misalign == "sh" else 0) and grad_sh.ptr % 16 == (4 if misalign == "grad_sh" else 0)
    assert lib.wg_eval_sh_forward(P, deg, K, d_sh.ptr, d_dirs.ptr, out.ptr, None) == 0
    assert lib.wg_eval_sh_backward(P, deg, K, d_sh.ptr, d_dirs.ptr, d_cot.ptr, grad_sh.ptr, grad_dirs.ptr if want_dirs else None, None) == 0
    torch.cuda.synchronize()
    got = {"out": out.values().reshape(P, 3), "grad_sh": grad_sh.values().reshape(P, 3, K)}
    out.assert_guards_intact("out")
    grad_sh.assert_guards_intact("grad_sh")
    if want_dirs:
        got["grad_dirs"] = grad_dirs.values().reshape(P, 3)
        grad_dirs.assert_guards_intact("grad_dirs")
    for name, r in (("sh", d_sh), ("dirs", d_dirs), ("grad_out", d_cot)):
        r.assert_unchanged(name)
    return got


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _record(forward_path, backward_path, ratios):
    """WG_WRITE_PROFILES=1: keep the largest error / bound per kernel path and tensor in profiles/sh_eval/accuracy.json.  The gate is the
    derived bound (ratio <= 1, asserted by the checker); the file only records where the kernels sit."""
    if os.environ.get("WG_WRITE_PROFILES") != "1":
        return
    path = os.path.join(ROOT, "profiles", "sh_eval", "accuracy.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {
        "metric": "sh_eval_accuracy", "yardstick": "max over all elements of |kernel - float64 oracle| / the element's a-priori float32 rounding "
        "bound (tests/sh_eval_lib.py); the gate (tests/test_sh_eval_edges.py) is 1 for every element",
        "device": torch.cuda.get_device_name(0), "paths": {}}
    for kernel, tensors in (("forward_" + forward_path, ("out",)), ("backward_" + backward_path, ("grad_sh", "grad_dirs"))):
        slot = data["paths"].setdefault(kernel, {})
        for t in tensors:
            if t in ratios:
                slot[t] = max(slot.get(t, 0.0), ratios[t])
    data["largest"] = max(max(r.values()) for r in data["paths"].values())
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_kernels_within_the_bounds_at_wave_alignment_and_degree_edges(case):
    sh, dirs, cot = L.case_inputs(case)
    got = _run(case.P, case.deg, case.K, sh, dirs, cot, misalign=case.misalign)
    ratios = L.check(got, case.deg, sh, dirs, cot)
    print(L.case_id(case), ratios)
    _record(L.kernel_path(case), L.kernel_path(case, backward=True), ratios)
    without = _run(case.P, case.deg, case.K, sh, dirs, cot, misalign=case.misalign, want_dirs=False)   # grad_dirs == NULL
    assert _same_bits(without["grad_sh"], got["grad_sh"]) and _same_bits(without["out"], got["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [None, "sh"], ids=["k16", "generic"])
def test_one_hot_coefficients_hold_every_basis_term_and_monomial_on_its_own(misalign):
    """One non-zero coefficient a row: the bound is a few ulps of that one term, over the whole mix of directions."""
    sh, dirs, cot = L.one_hot_inputs()
    got = _run(192, 3, 16, sh, dirs, cot, misalign=misalign)
    ratios = L.check(got, 3, sh, dirs, cot)
    path = "k16" if misalign is None else "generic_scalar"
    _record(path, path, ratios)


POISONED_ROWS = (64, 127, 190)   # of P = 191: lane 0 and lane 63 of the second wave, the last valid lane of the partial third one


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 20])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_nan_at_an_inactive_coefficient_changes_nothing(deg, K):
    n = L.n_coefficients(deg)
    sh, dirs, cot = L.coefficients(191, K, 40 + deg), L.directions(191, 40 + deg), L.cotangent(191, 40 + deg)
    clean = _run(191, deg, K, sh, dirs, cot)
    poisoned = sh.copy()
    poisoned[list(POISONED_ROWS), :, n:] = np.nan
    got = _run(191, deg, K, poisoned, dirs, cot)
    L.check(got, deg, sh, dirs, cot)   # against an oracle that never sees the NaN
    assert not any(np.isnan(t).any() for t in got.values()) and not got["grad_sh"][:, :, n:].any()
    assert all(_same_bits(got[t], clean[t]) for t in got)


@pytest.mark.gpu
@pytest.mark.parametrize("K,misalign", [(16, None), (16, "sh"), (20, None)], ids=["k16", "generic_scalar", "generic_vec16"])
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_nan_at_an_active_coefficient_stays_in_its_row(deg, K, misalign):
    """out is NaN for exactly that row and channel, grad_dirs for exactly that row, grad_sh (which does not read sh) nowhere; every other
    row of the same wave stays within its bound.  The poisoned coefficient is one the direction's gradient reads."""
    k = {1: 2, 2: 6, 3: 6}[deg]
    sh, dirs, cot = L.coefficients(191, K, 50 + deg), L.directions(191, 50 + deg), L.cotangent(191, 50 + deg)
    for r in POISONED_ROWS:
        sh[r, r % 3, k] = np.nan
    got = _run(191, deg, K, sh, dirs, cot, misalign=misalign)
    L.check(got, deg, sh, dirs, cot)   # NaN exactly where the oracle has it, the bound everywhere else
    assert np.argwhere(np.isnan(got["out"])).tolist() == [[r, r % 3] for r in POISONED_ROWS]
    assert np.flatnonzero(np.isnan(got["grad_dirs"]).any(axis=1)).tolist() == list(POISONED_ROWS)
    assert not np.isnan(got["grad_sh"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [L.Case(191, 3, 16, None), L.Case(257, 2, 16, "sh"), L.Case(257, 3, 20, None), L.Case(191, 3, 25, None)],
                         ids=L.case_id)
def test_two_calls_give_identical_bits(case):
    sh, dirs, cot = L.case_inputs(case)
    a = _run(case.P, case.deg, case.K, sh, dirs, cot, misalign=case.misalign)
    b = _run(case.P, case.deg, case.K, sh, dirs, cot, misalign=case.misalign)
    assert all(_same_bits(a[t], b[t]) for t in L.TENSORS)


@pytest.mark.gpu
def test_argument_rules_of_the_header():
    lib = _lib()
    r = _Region(64 * 3 * 16)
    p = r.ptr
    fwd = lambda P, deg, K, sh=p, dirs=p, out=p: lib.wg_eval_sh_forward(P, deg, K, sh, dirs, out, None)
    bwd = lambda P, deg, K, sh=p, dirs=p, g=p, gsh=p, gd=p: lib.wg_eval_sh_backward(P, deg, K, sh, dirs, g, gsh, gd, None)
    for call in (fwd, bwd):
        assert call(-1, 3, 16) == -1      # negative P
        assert call(4, 4, 25) == -1       # degree 4
        assert call(4, -1, 16) == -1
        for deg in (1, 2, 3):
            assert call(4, deg, (deg + 1) ** 2 - 1) == -1   # K < N
        assert call(4, 3, 16, sh=None) == -1 and call(4, 3, 16, dirs=None) == -1
    assert fwd(4, 3, 16, out=None) == -1
    assert bwd(4, 3, 16, g=None) == -1 and bwd(4, 3, 16, gsh=None) == -1
    assert lib.wg_eval_sh_forward(0, 3, 16, None, None, None, None) == 0    # P = 0 with NULL pointers
    assert lib.wg_eval_sh_backward(0, 3, 16, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    r.assert_unchanged("a refused call's buffer")


# ---- GPU: the wrapper (wg_fused_gaussians.eval_sh) -----------------------------------------------------------------------------------
def _cuda(a, grad=False):
    return torch.from_numpy(a).cuda().requires_grad_(grad)


def _wrapper_inputs(P, seed, K=16):
    return L.coefficients(P, K, seed), L.directions(P, seed), L.cotangent(P, seed)


@pytest.mark.gpu
def test_wrapper_leading_batch_dimensions():
    from wg_fused_gaussians import eval_sh
    sh, dirs, cot = _wrapper_inputs(10, 60)
    t_sh, t_dirs = _cuda(sh.reshape(2, 5, 3, 16), True), _cuda(dirs.reshape(2, 5, 3), True)
    out = eval_sh(3, t_sh, t_dirs)
    assert out.shape == (2, 5, 3)
    out.backward(_cuda(cot.reshape(2, 5, 3)))
    assert t_sh.grad.shape == (2, 5, 3, 16) and t_dirs.grad.shape == (2, 5, 3)
    L.check({"out": out.detach().cpu().numpy().reshape(10, 3), "grad_sh": t_sh.grad.cpu().numpy().reshape(10, 3, 16),
             "grad_dirs": t_dirs.grad.cpu().numpy().reshape(10, 3)}, 3, sh, dirs, cot)


@pytest.mark.gpu
def test_wrapper_callers_transposed_view_sends_the_gradient_to_the_leaf():
    """features.view(-1, 16, 3).transpose(1, 2) without .contiguous() (method.py:1558-1565)."""
    from wg_fused_gaussians import eval_sh
    P = 65
    sh, dirs, cot = _wrapper_inputs(P, 61)
    feats = _cuda(np.ascontiguousarray(sh.transpose(0, 2, 1)).reshape(P, 48), True)
    view = feats.view(-1, 16, 3).transpose(1, 2)
    assert not view.is_contiguous()
    t_dirs = _cuda(dirs, True)
    out = eval_sh(3, view, t_dirs)
    out.backward(_cuda(cot))
    assert feats.grad.shape == (P, 48)
    L.check({"out": out.detach().cpu().numpy(), "grad_sh": feats.grad.view(P, 16, 3).transpose(1, 2).cpu().numpy(),
             "grad_dirs": t_dirs.grad.cpu().numpy()}, 3, sh, dirs, cot)


@pytest.mark.gpu
def test_wrapper_contiguous_view_at_a_four_byte_storage_offset():
    """Reaches the generic kernel through the wrapper: the view is contiguous, so the wrapper passes its pointer on as it is."""
    from wg_fused_gaussians import eval_sh
    P = 65
    sh, dirs, cot = _wrapper_inputs(P, 62)
    store = torch.zeros(P * 48 + 1, device="cuda")
    store[1:] = torch.from_numpy(sh).cuda().reshape(-1)
    t_sh = store[1:].view(P, 3, 16).requires_grad_(True)
    assert t_sh.is_contiguous() and t_sh.data_ptr() % 16 == 4
    t_dirs = _cuda(dirs, True)
    out = eval_sh(3, t_sh, t_dirs)
    out.backward(_cuda(cot))
    ratios = L.check({"out": out.detach().cpu().numpy(), "grad_sh": t_sh.grad.cpu().numpy(), "grad_dirs": t_dirs.grad.cpu().numpy()}, 3, sh, dirs, cot)
    _record("generic_scalar", "generic_scalar", ratios)


@pytest.mark.gpu
@pytest.mark.parametrize("needs", ["sh", "dirs", "neither"])
def test_wrapper_gradients_only_where_they_are_asked_for(needs):
    from wg_fused_gaussians import eval_sh
    P = 65
    sh, dirs, cot = _wrapper_inputs(P, 63)
    t_sh, t_dirs = _cuda(sh, needs == "sh"), _cuda(dirs, needs == "dirs")
    other = torch.ones(P, 3, device="cuda", requires_grad=True)
    out = eval_sh(2, t_sh, t_dirs)
    (out * other).backward(_cuda(cot))   # a sum with another leaf must not raise, whoever asks for a gradient
    got = {"out": out.detach().cpu().numpy()}
    if needs == "sh":
        got["grad_sh"] = t_sh.grad.cpu().numpy()
    if needs == "dirs":
        got["grad_dirs"] = t_dirs.grad.cpu().numpy()
    assert (t_sh.grad is None) == (needs != "sh") and (t_dirs.grad is None) == (needs != "dirs")
    assert len(L.check(got, 2, sh, dirs, cot)) == (1 if needs == "neither" else 2)
    assert _same_bits(other.grad.cpu().numpy(), (out.detach() * _cuda(cot)).cpu().numpy())


@pytest.mark.gpu
def test_wrapper_no_rows():
    from wg_fused_gaussians import eval_sh
    t_sh, t_dirs = torch.zeros(0, 3, 16, device="cuda", requires_grad=True), torch.zeros(0, 3, device="cuda", requires_grad=True)
    out = eval_sh(3, t_sh, t_dirs)
    assert out.shape == (0, 3)
    out.sum().backward()
    assert t_sh.grad.shape == (0, 3, 16) and t_dirs.grad.shape == (0, 3)
    empty = np.zeros((0, 3), np.float32)
    L.check({"out": out.detach().cpu().numpy(), "grad_sh": t_sh.grad.cpu().numpy(), "grad_dirs": t_dirs.grad.cpu().numpy()}, 3,
            np.zeros((0, 3, 16), np.float32), empty, empty)


@pytest.mark.gpu
def test_wrapper_degree_as_a_device_tensor_and_a_non_contiguous_grad_out():
    from wg_fused_gaussians import eval_sh
    P = 191
    sh, dirs, cot = _wrapper_inputs(P, 64)
    t_sh, t_dirs = _cuda(sh, True), _cuda(dirs, True)
    out = eval_sh(torch.tensor(1, device="cuda"), t_sh, t_dirs)   # the caller's `active_sh_degree` buffer
    grad_out = _cuda(np.ascontiguousarray(cot.T)).t()
    assert not grad_out.is_contiguous()
    out.backward(grad_out)
    L.check({"out": out.detach().cpu().numpy(), "grad_sh": t_sh.grad.cpu().numpy(), "grad_dirs": t_dirs.grad.cpu().numpy()}, 1, sh, dirs, cot)
