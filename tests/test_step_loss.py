"""Fused train-step image loss (include/wg_step_loss.h, csrc/loss/step_loss.hip, wg_fused_ssim.step_loss / step_metrics) against the
reference's own statements (wildgaussians/method.py:1920-1992).

Oracle: tests/step_loss_lib.py's float64 restatement, pinned on the CPU to 1e-12 of the float64 values and gradients recorded from the
reference's statements in tests/golden/step_loss_ref.npz.
Values: every stats entry and the loss are held to 4 * max(ref32_dev, 16 float32 ulps of the oracle's value), ref32_dev = |the reference's own
float32 result - its float64 result| for that entry on that input: recorded in the fixture for its cases, taken from the restatement run in
float32 on the same inputs for shapes generated here (the gate of tests/test_uncertainty.py and tests/test_lpips.py).  Entries that are NaN or
infinite in the oracle must be that exactly.
Gradients: max |kernel - oracle| <= 1e-4 of the oracle gradient's largest magnitude (tests/test_ssim.py's bound for this backward arithmetic).
The effective multiplier is held bit for bit through the gradient of a frame whose L1 term alone is active.
WG_WRITE_PROFILES=1 records the measured ratios in profiles/step_loss/accuracy.json.
"""
import ctypes as C
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_loss_lib as L  # noqa: E402

GOLDEN = L.load_golden()
IDS = [c["name"] for c, _ in GOLDEN]
LIB = os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so")
N = len(L.STATS)


def ulp16(v):
    return 16 * float(np.spacing(np.float32(abs(v))))


def stat_ratios(got, ref64, ref32):
    """Per entry |got - ref64| / max(|ref32 - ref64|, 16 ulps): the gate is 4.  Non-finite oracle entries must be matched exactly (ratio 0)."""
    out = {}
    for k, name in enumerate(L.STATS):
        g, r, r32 = float(got[k]), float(ref64[k]), float(ref32[k])
        if not np.isfinite(r):
            assert (np.isnan(g) and np.isnan(r)) or g == r, (name, g, r)
            out[name] = 0.0
        else:
            assert np.isfinite(g), (name, g, r)
            out[name] = abs(g - r) / max(abs(r32 - r) if np.isfinite(r32) else 0.0, ulp16(r))
    return out


def grad_ratio(got, ref64):
    """max |got - ref| / (1e-4 * max |ref|): the gate is 1.  A gradient that is zero in the oracle must be zero."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    err, top = np.abs(got - ref64).max(), np.abs(ref64).max()
    if top == 0:
        assert err == 0
        return 0.0
    return float(err / (1e-4 * top))


def _record(case, ratios):
    if os.environ.get("WG_WRITE_PROFILES") != "1":
        return
    path = os.path.join(ROOT, "profiles", "step_loss", "accuracy.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {
        "metric": "step_loss_accuracy", "yardstick": "stats and loss: |kernel - float64 oracle| / max(ref32_dev, 16 float32 ulps of the value), "
        "ref32_dev = the reference statements' own |float32 - float64| on the same input, gate 4; grad_*: max |kernel - oracle| / (1e-4 * the "
        "oracle gradient's largest magnitude), gate 1 (tests/test_step_loss.py)", "device": torch.cuda.get_device_name(0), "cases": {}}
    data["cases"][case] = ratios
    data["largest_stat_ratio"] = max(v for r in data["cases"].values() for k, v in r.items() if not k.startswith("grad_"))
    data["largest_grad_ratio"] = max(v for r in data["cases"].values() for k, v in r.items() if k.startswith("grad_"))
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------- CPU: the fixture, the oracle, the exports, the argument checks

def test_fixture_holds_the_cases_of_the_helper():
    assert [c for c, _ in GOLDEN] == [dict(c) for c in L.CASES]
    assert os.path.getsize(L.GOLDEN) <= 1 << 20
    for c, a in GOLDEN:
        Cn, H, W = c["shape"]
        assert H <= 45 and W <= 70
        for k in ("toned", "raw", "gt"):
            assert a[k].dtype == np.float32 and a[k].shape == c["shape"]
        assert ("mask" in a) == (c["mask"] != "none") and ("mult" in a) == (c["schedule"] is not None)
        for p, dt in (("32", np.float32), ("64", np.float64)):
            assert a["stats" + p].shape == (N,) and a["stats" + p].dtype == np.float64
            assert a["grad_toned" + p].dtype == dt and a["grad_raw" + p].dtype == dt
            assert np.isnan(a["stats" + p][7:]).all() == (c["mask"] == "none")
    blends = [L.blend_of(c["schedule"]) for c, _ in GOLDEN if c["schedule"] is not None]
    assert 0.0 in blends and 1.0 in blends and any(0 < b < 1 for b in blends)          # before, during and after the warm-up
    assert {c["mask"] for c, _ in GOLDEN} >= {"none", "binary", "fractional"} and any(c["shape"][0] != 3 for c, _ in GOLDEN)
    assert any(np.isnan(a["mult"]).any() and (a["mult"] == 1.0).any() for _, a in GOLDEN if "mult" in a)


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=IDS)
def test_float64_oracle_reproduces_the_recorded_reference_statements(i):
    c, a = GOLDEN[i]
    t = lambda k: torch.from_numpy(a[k]) if k in a else None  # noqa: E731
    o = L.oracle(t("toned"), t("raw"), t("gt"), t("mask"), t("mult"), **L.case_kwargs(c))
    got, ref = L.stats_vector(o["stats"]), a["stats64"]
    assert (np.isnan(got) == np.isnan(ref)).all()
    assert np.nanmax(np.abs(got - ref)) <= 1e-12
    assert np.abs(o["grad_toned"].numpy() - a["grad_toned64"]).max() <= 1e-12 and np.abs(o["grad_raw"].numpy() - a["grad_raw64"]).max() <= 1e-12
    # the normalisation that is easy to get wrong: masked MSE and L1 sum the three channels and divide by mask.sum() alone
    if "mask" in a:
        k, d = a["mask"].astype(np.float64), a["toned"].astype(np.float64) - a["gt"].astype(np.float64)
        assert abs((d * d * k).sum() / k.sum() - ref[L.STATS.index("mse_masked")]) <= 1e-12
        assert abs((np.abs(d) * k).sum() / k.sum() - ref[L.STATS.index("l1_loss_masked")]) <= 1e-12


def test_c_abi_exports_the_step_loss_entry_points():
    lib = C.CDLL(LIB)
    hdr = open(os.path.join(ROOT, "include", "wg_step_loss.h")).read()
    names = set(re.findall(r"\b(wg_step_loss_\w+)\s*\(", hdr))
    assert names == {"wg_step_loss_scratch_floats", "wg_step_loss_forward", "wg_step_loss_backward"}
    for n in names:
        assert hasattr(lib, n), n
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(WG_STEP_\w+) = (\d+)", hdr))
    assert enum.pop("WG_STEP_STATS") == N and sorted(enum.values()) == list(range(N))
    lib.wg_step_loss_scratch_floats.restype = C.c_size_t
    assert lib.wg_step_loss_scratch_floats(3, 1200, 1600) == 18 * 50 * 75 * 3
    assert lib.wg_step_loss_scratch_floats(3, 17, 33) == 18 * 2 * 2 * 3
    for bad in ((0, 4, 4), (3, 0, 4), (3, 4, -1), (65536, 4, 4)):
        assert lib.wg_step_loss_scratch_floats(*bad) == 0


def _abi():
    lib = C.CDLL(LIB)
    vp, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double
    lib.wg_step_loss_forward.restype = i
    lib.wg_step_loss_forward.argtypes = [i, i, i] + [vp] * 5 + [i, f, f, d] + [vp] * 7
    lib.wg_step_loss_backward.restype = i
    lib.wg_step_loss_backward.argtypes = [i, i, i] + [vp] * 5 + [i, f, f, d] + [vp] * 7
    return lib


def test_c_abi_refuses_malformed_calls_before_any_launch():
    """Every call below is refused by the argument checks, which come before any device work: the pointers are never read (they are not even
    device addresses), and no device is needed."""
    lib = _abi()
    P = [0x1000 * (k + 1) for k in range(12)]   # distinct, 8-byte aligned, never dereferenced
    sched = (1, 1.0, 0.5, 0.2)

    def fwd(size=(3, 8, 8), l1=P[0], ss=P[1], gt=P[2], mask=P[3], mult=P[4], scratch=P[5], loss=P[6], stats=P[7], maps=(P[8], P[9], P[10])):
        return lib.wg_step_loss_forward(*size, l1, ss, gt, mask, mult, *sched, scratch, loss, stats, *maps, None)

    def bwd(size=(3, 8, 8), l1=P[0], ss=P[1], gt=P[2], mask=P[3], mult=P[4], gl=P[5], maps=(P[8], P[9], P[10]), g_l1=P[6], g_ss=P[7]):
        return lib.wg_step_loss_backward(*size, l1, ss, gt, mask, mult, *sched, gl, *maps, g_l1, g_ss, None)

    for size in ((0, 8, 8), (3, 0, 8), (3, 8, 0), (-1, 8, 8), (65536, 8, 8)):
        assert fwd(size=size) == -1 and bwd(size=size) == -1
    for name in ("l1", "ss", "gt", "scratch", "loss", "stats"):
        assert fwd(**{name: None}) == -1, name
    assert fwd(scratch=P[5] + 4) == -1 and fwd(stats=P[7] + 4) == -1                      # the float64 buffers must be 8-byte aligned
    for maps in ((P[8], None, None), (None, P[9], P[10]), (P[8], P[9], None), (P[8], None, P[10])):   # all three or none
        assert fwd(maps=maps) == -1, maps
    for name in ("l1", "ss", "gt", "gl", "g_l1", "g_ss"):
        assert bwd(**{name: None}) == -1, name
    for maps in ((None, P[9], P[10]), (P[8], None, P[10]), (P[8], P[9], None), (None, None, None)):   # the backward needs all three
        assert bwd(maps=maps) == -1, maps
    assert bwd(ss=P[0]) == -1                  # one image, two gradients
    assert bwd(g_ss=P[6]) == -1                # two images, one gradient


# ---------------------------------------------------------------- GPU

def _dev(t):
    return None if t is None else t.to("cuda:0")


def run_fused(toned, raw, gt, mask, mult, lam=L.LAMBDA, threshold=None, blend=1.0, one_image=False, grad_scale=1.0):
    """step_loss forward and backward on the device: (loss float, stats float64 [N], grad_toned, grad_raw or None) as NumPy."""
    from wg_fused_ssim import step_loss
    a = _dev(toned).clone().requires_grad_(True)
    b = a if one_image else _dev(raw).clone().requires_grad_(True)
    loss, stats = step_loss(a, b, _dev(gt), lam, mask=_dev(mask), loss_mult=_dev(mult), mult_threshold=threshold, mult_blend=blend)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    assert stats.dtype == torch.float64 and stats.shape == (N,) and not stats.requires_grad
    (loss * grad_scale).backward()
    return float(loss.item()), stats.cpu().numpy(), a.grad.cpu().numpy(), None if one_image else b.grad.cpu().numpy()


def check_against_oracle(label, got, o64, s32):
    """The value gate and the gradient gate; returns the ratios (and records them)."""
    loss, stats, g_toned, g_raw = got
    s64 = L.stats_vector(o64["stats"]) if isinstance(o64["stats"], dict) else o64["stats"]
    ratios = stat_ratios(stats, s64, s32)
    assert loss == float(np.float32(stats[0]))        # the float32 loss is the float64 one, rounded once
    ratios["grad_toned"] = grad_ratio(g_toned, o64["grad_toned"])
    if g_raw is not None:
        ratios["grad_raw"] = grad_ratio(g_raw, o64["grad_raw"])
    print(label, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    _record(label, ratios)
    bad = {k: v for k, v in ratios.items() if v > (1.0 if k.startswith("grad_") else 4.0)}
    assert not bad, (label, bad)
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=IDS)
def test_recorded_cases_within_four_times_the_reference_float32_error(i):
    c, a = GOLDEN[i]
    t = lambda k: torch.from_numpy(a[k]) if k in a else None  # noqa: E731
    kw = L.case_kwargs(c)
    got = run_fused(t("toned"), t("raw"), t("gt"), t("mask"), t("mult"), **kw)
    check_against_oracle("golden/" + c["name"], got, {"stats": a["stats64"], "grad_toned": a["grad_toned64"], "grad_raw": a["grad_raw64"]},
                         a["stats32"])


MULTS = {   # name -> (kind, threshold, blend)
    "no_mult": (None, None, 1.0),
    "raw_blend0": ("raw", 1.0, 0.0),
    "raw_blend037": ("raw", 1.0, 0.37),
    "raw_blend1": ("raw", 1.0, 1.0),
    "ready_made": ("ready", None, 1.0),
}


@functools.lru_cache(maxsize=None)
def generated(shape, mask_kind, mult_name, one_image=False):
    """Inputs, the float64 oracle and the float32 restatement's stats of a generated case, computed once on the CPU."""
    kind, threshold, blend = MULTS[mult_name]
    toned, raw, gt, mask, mult = L.make_inputs(shape, mask_kind, kind is not None, seed=sum(shape) + 31 * len(mask_kind) + len(mult_name))
    if kind == "ready":   # a ready-made fractional multiplier: no NaN, nothing to threshold
        mult = torch.nan_to_num(mult, nan=0.25)
    kw = {"threshold": threshold, "blend": blend, "one_image": one_image}
    o64 = L.oracle(toned, raw, gt, mask, mult, **kw)
    s32 = L.stats_vector(L.statements(toned, raw, gt, mask, mult, **kw)["stats"])
    return (toned, raw, gt, mask, mult), kw, o64, s32


# (3, 1, 1), (3, 7, 5): smaller than the window.  (3, 16, 32): exactly one tile.  (3, 17, 33): one pixel over in both axes, four ragged workgroups
# per plane.  (1, 33, 47): C != 3 changes ssim_masked's divisor.  (3, 304, 608): 19 * 19 * 3 = 1083 workgroups, more than the finishing kernel's
# 1024 threads.
SHAPES = [(3, 1, 1), (3, 7, 5), (3, 16, 32), (3, 17, 33), (3, 45, 70), (1, 33, 47), (3, 304, 608)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", ["plain", "masked_warmup"])
def test_shapes_within_the_gate(shape, variant):
    mask_kind, mult_name = ("none", "no_mult") if variant == "plain" else ("fractional", "raw_blend037")
    inputs, kw, o64, s32 = generated(shape, mask_kind, mult_name)
    check_against_oracle(f"shape/{'x'.join(map(str, shape))}/{variant}", run_fused(*inputs, **kw), o64, s32)


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["none", "ones", "binary", "fractional", "zeros"])
@pytest.mark.parametrize("mult_name", list(MULTS))
def test_masks_and_multipliers_within_the_gate(mask_kind, mult_name):
    inputs, kw, o64, s32 = generated((3, 17, 33), mask_kind, mult_name)
    got = run_fused(*inputs, **kw)
    check_against_oracle(f"mask/{mask_kind}/{mult_name}", got, o64, s32)
    stats = got[1]
    if mask_kind == "none":
        assert np.isnan(stats[7:]).all() and np.isfinite(stats[:7]).all()
    elif mask_kind == "zeros":   # NaN in exactly the four ratios; the gradients of a fully masked frame are zero
        assert stats[7] == 0.0 and np.isnan(stats[8:]).all() and np.isfinite(stats[:7]).all()
        assert not got[2].any() and not got[3].any()
    else:
        assert np.isfinite(stats).all()
        if mask_kind == "ones":
            assert stats[7] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["none", "fractional"])
@pytest.mark.parametrize("blend", [0.0, 0.37, 1.0])
def test_effective_multiplier_has_the_bits_of_the_pytorch_expression(mask_kind, blend):
    """lambda = 0 and grad_output = C*H*W: |grad_toned| is then the effective multiplier times the mask, rounded once."""
    shape = (3, 17, 33)
    toned, raw, gt, mask, mult = L.make_inputs(shape, mask_kind, True, seed=77)
    assert torch.isnan(mult).any() and (mult == 1.0).any() and (mult > 1).any() and (mult < 1).any() and ((toned - gt) != 0).all()
    chw = float(np.prod(shape))
    _, _, g_toned, g_raw = run_fused(toned, raw, gt, mask, mult, lam=0.0, threshold=1.0, blend=blend, grad_scale=chw)
    expected = 1 + blend * ((mult > 1).float() - 1)          # method.py:1934 and :1940 in float32 PyTorch
    if mask is not None:
        expected = expected * mask
    expected = expected.expand(shape).numpy()
    assert expected.dtype == np.float32
    assert np.array_equal(np.abs(g_toned), expected)
    assert np.array_equal(np.sign(g_toned), (np.sign((toned - gt).numpy()) * (expected != 0)).astype(np.float32))
    assert not g_raw.any()                                    # the SSIM term is switched off


@pytest.mark.gpu
def test_one_image_gives_one_summed_gradient():
    inputs, kw, o64, s32 = generated((3, 17, 33), "binary", "raw_blend037", True)
    got = run_fused(*inputs, **kw)
    assert got[3] is None
    check_against_oracle("contract/one_image", got, o64, s32)


@pytest.mark.gpu
def test_identical_images_give_zero_mse_infinite_psnr_and_ssim_one():
    from wg_fused_ssim import step_loss, step_metrics
    gt = L.make_inputs((3, 45, 70), "none", False, seed=5)[2].to("cuda:0")
    x = gt.clone().requires_grad_(True)
    loss, stats = step_loss(x, x, gt)
    m = step_metrics(stats)
    assert m["mse"] == 0.0 and m["l1_loss"] == 0.0 and m["psnr"] == float("inf") and abs(m["ssim"] - 1.0) <= 1e-5
    loss.backward()
    assert torch.isfinite(x.grad).all()


@pytest.mark.gpu
def test_two_calls_give_identical_bits_and_no_grad_allocates_no_maps():
    from wg_fused_ssim import step_loss
    shape = (3, 304, 608)
    (toned, raw, gt, mask, mult), kw, _, _ = generated(shape, "fractional", "raw_blend037")
    a, b = run_fused(toned, raw, gt, mask, mult, **kw), run_fused(toned, raw, gt, mask, mult, **kw)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    dt, dr, dg, dk, dm = (_dev(t) for t in (toned, raw, gt, mask, mult))
    dt.requires_grad_(True)
    maps_bytes = 3 * int(np.prod(shape)) * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        return torch.cuda.max_memory_allocated() - base, out

    call = lambda: step_loss(dt, dr, dg, L.LAMBDA, mask=dk, loss_mult=dm, mult_threshold=1.0, mult_blend=0.37)  # noqa: E731
    with torch.no_grad():
        used, (loss, stats) = peak(call)
    assert used < maps_bytes // 3 and not loss.requires_grad            # scratch, loss and stats only
    assert stats.cpu().numpy().tobytes() == a[1].tobytes() and float(loss.item()) == a[0]
    used, (loss, _) = peak(call)
    assert used >= maps_bytes and loss.requires_grad


@pytest.mark.gpu
def test_plain_case_agrees_with_l1_ssim_loss():
    """Without mask and multiplier the loss, l1_loss and ssim are what l1_ssim_loss(..., return_parts=True) returns, within the value gate."""
    from wg_fused_ssim import l1_ssim_loss, step_loss
    c, a = GOLDEN[0]
    assert c["mask"] == "none" and c["schedule"] is None
    toned, raw, gt = (torch.from_numpy(a[k]).to("cuda:0") for k in ("toned", "raw", "gt"))
    loss, stats = step_loss(toned, raw, gt, L.LAMBDA)
    ref = [float(v.item()) for v in l1_ssim_loss(toned, raw, gt, L.LAMBDA, return_parts=True)]
    stats = stats.cpu().numpy()
    for k, r in zip((0, 1, 2), ref):
        bound = 4 * max(abs(a["stats32"][k] - a["stats64"][k]), ulp16(a["stats64"][k]))
        assert abs(stats[k] - r) <= bound, (L.STATS[k], stats[k], r, bound)
    assert abs(float(loss.item()) - ref[0]) <= 4 * ulp16(ref[0])


@pytest.mark.gpu
def test_step_metrics_returns_the_reference_key_set_and_constants_are_refused():
    from wg_fused_ssim import step_loss, step_metrics
    toned, raw, gt, mask, mult = (_dev(t) for t in L.make_inputs((3, 17, 33), "binary", True, seed=9))
    _, stats = step_loss(toned, raw, gt, 0.2, loss_mult=mult, mult_threshold=1)
    m = step_metrics(stats)
    assert set(m) == set(L.LOGGED) and all(type(v) is float for v in m.values())
    _, stats = step_loss(toned, raw, gt, 0.2, mask=mask[0], loss_mult=mult[0], mult_threshold=1)     # [H, W] planes
    m = step_metrics(stats, prefix="train/")
    assert set(m) == {"train/" + k for k in L.LOGGED + L.LOGGED_MASKED} and all(type(v) is float for v in m.values())
    assert m["train/mask_percentage"] == float(mask.double().sum().item()) / (17 * 33)   # a 0/1 mask: the sum is exact
    for bad in ({"mask": mask.clone().requires_grad_(True)}, {"loss_mult": mult.clone().requires_grad_(True)}, {"mask": mask[:, :-1]},
                {"loss_mult": mult.expand(3, -1, -1)}, {"mask": mask.cpu()}):
        with pytest.raises(RuntimeError):
            step_loss(toned, raw, gt, 0.2, **bad)
    with pytest.raises(RuntimeError):
        step_loss(toned, raw, gt.clone().requires_grad_(True), 0.2)


@pytest.mark.gpu
def test_guard_words_around_scratch_stats_and_gradients_stay_untouched():
    """The C-ABI on buffers carved out of larger ones: the words before and after the scratch, the stats vector and both gradients keep their fill."""
    import wg_fused_ssim as S
    from diff_gaussian_rasterization import _C as native
    shape = (3, 17, 33)
    Cn, H, W = shape
    n = int(np.prod(shape))
    toned, raw, gt, mask, mult = (_dev(t).contiguous() for t in L.make_inputs(shape, "fractional", True, seed=11))
    G, FILL = 64, -12345.0
    words = S._lib.wg_step_loss_scratch_floats(Cn, H, W)
    assert words == 18 * 2 * 2 * 3

    def guarded(count, dtype):
        buf = torch.full((G + count + G,), FILL, device="cuda:0", dtype=dtype)
        return buf, buf[G:G + count]

    scratch_buf, scratch = guarded(words // 2, torch.float64)
    stats_buf, stats = guarded(N, torch.float64)
    loss_buf, loss = guarded(1, torch.float32)
    maps = torch.empty((3, n), device="cuda:0")
    ga_buf, ga = guarded(n, torch.float32)
    gb_buf, gb = guarded(n, torch.float32)
    gl = torch.ones(1, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    sched = (1, 1.0, 0.37, 0.2)
    native._check(S._lib.wg_step_loss_forward(Cn, H, W, toned.data_ptr(), raw.data_ptr(), gt.data_ptr(), mask.data_ptr(), mult.data_ptr(), *sched,
                                              scratch.data_ptr(), loss.data_ptr(), stats.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                              maps[2].data_ptr(), stream), "wg_step_loss_forward")
    native._check(S._lib.wg_step_loss_backward(Cn, H, W, toned.data_ptr(), raw.data_ptr(), gt.data_ptr(), mask.data_ptr(), mult.data_ptr(), *sched,
                                               gl.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), ga.data_ptr(),
                                               gb.data_ptr(), stream), "wg_step_loss_backward")
    torch.cuda.synchronize()
    for buf, inner in ((scratch_buf, scratch), (stats_buf, stats), (loss_buf, loss), (ga_buf, ga), (gb_buf, gb)):
        assert (buf[:G] == FILL).all() and (buf[G + inner.numel():] == FILL).all()
        assert (inner != FILL).all()                                    # and everything between them was written
    _, ref_stats, ref_ga, ref_gb = run_fused(toned.cpu(), raw.cpu(), gt.cpu(), mask.cpu(), mult.cpu(), threshold=1.0, blend=0.37)
    assert stats.cpu().numpy().tobytes() == ref_stats.tobytes()
    assert np.array_equal(ga.cpu().numpy().reshape(shape), ref_ga) and np.array_equal(gb.cpu().numpy().reshape(shape), ref_gb)
