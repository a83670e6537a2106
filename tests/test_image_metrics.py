"""Fused evaluation metrics (include/wg_metrics.h, wg_fused_metrics, wg_integration.fuse_evaluation_metrics) against the reference's
per-image chain: render() -> image_to_srgb(uint8) -> compute_metrics (wildgaussians/evaluation.py:331-352).

Oracle: tests/image_metrics_lib.py, a NumPy restatement of that chain in the reference's operation order and dtypes (float32 values and
products, float64 taps, filtering and everything after), which tests/golden/image_metrics_ref.npz -- numbers recorded from the reference's
own functions -- pins on the CPU.

Conditions, derived and not measured:
  SSIM       |fused - oracle| <= 1e-10.  22 double taps and the products give at most about 24 roundings of 2^-53 on values <= 1, so a variance
             term is off by less than 1e-14; the expression's sensitivity to it is at most 2 / c2 = 2.2e3, over three such terms: under 1e-10
             per pixel, and the mean is no worse.  max, min and sign are continuous where they switch.
  MSE, MAE   relative <= 1e-9: the worst case of reordering a double sum of up to 2^23 non-negative terms whose float32 inputs are identical;
             exactly 0 where the oracle is 0.
  PSNR       -10 log10 of the returned mse, inf for equal images.
  quantize   equality of bits.
"""
import ctypes as C
import inspect
import math
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import image_metrics_lib as L  # noqa: E402

REFERENCE = "/root/reference"
DEV = "cuda:0"
gpu = pytest.mark.gpu
SSIM_ABS, SUM_REL = 1e-10, 1e-9
SINGLE = [n for n in L.CASE_NAMES if n != "batch"]


@pytest.fixture(scope="module")
def golden():
    z = np.load(L.GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    """name -> (case, pred, gt, oracle), computed once and left unchanged."""
    out = {}
    for c in L.CASES:
        pred, gt = L.make_inputs(c)
        out[c["name"]] = (c, pred, gt, L.oracle(c, pred, gt))
        pred.setflags(write=False), gt.setflags(write=False)
    return out


def dbits(x):
    return struct.pack("<d", float(x))


def same_result_bits(a, b):
    return all(dbits(a[k]) == dbits(b[k]) for k in ("psnr", "ssim", "mae", "mse"))


# =============================================================================================== CPU
def test_fixture_is_small_and_matches_the_case_table(golden):
    import json
    assert os.path.getsize(L.GOLDEN) <= 1024 * 1024
    recorded = json.loads(str(golden["cases"]))
    mine = [dict(c, shape=list(c["shape"]), roi=list(c["roi"]) if c["roi"] else None) for c in L.CASES]
    assert recorded == mine
    for c in L.CASES:
        batch = tuple(c["shape"][:-3])
        for k in ("psnr", "ssim", "mae", "mse", "ssim64"):
            v = golden[f"{c['name']}__{k}"]
            assert v.dtype == np.float64 and v.shape == batch, (c["name"], k)
    assert int(golden["edge_count"]) == L.edge_floats().size == golden["edge_bytes"].size
    assert golden["edge_bytes"].dtype == np.uint8


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_oracle_reproduces_the_recording(golden, cases, name):
    """SSIM to 1e-12 absolute (the same operations; only the order of additions may differ); MSE and MAE within 2e-6 relative of the
    reference's float32 np.mean (its blocked pairwise sum: about 30 roundings of 2^-24)."""
    _, _, _, o = cases[name]
    assert np.all(np.abs(o["ssim"] - golden[name + "__ssim"]) <= 1e-12)
    for k in ("mse", "mae"):
        rec = golden[f"{name}__{k}"]
        assert np.all(np.abs(o[k] - rec) <= 2e-6 * np.abs(rec)), (k, o[k], rec)
        assert np.all((o[k] == 0) == (rec == 0))


def test_float32_products_are_part_of_the_reported_ssim(golden, cases):
    """The recorded dmpix_ssim on float64 copies of the inputs is what the oracle gives on such copies, and it is NOT the reported value:
    the float32 roundings of a*a, b*b, a*b move SSIM by up to 1e-6, far above the 1e-10 the fused operator is held to."""
    worst = 0.0
    for name in SINGLE:
        c, pred, gt, o = cases[name]
        a, b = L.prepare(c, pred, gt)
        all64 = np.mean(L.ssim_map(b.astype(np.float64), a.astype(np.float64)))
        assert abs(all64 - golden[name + "__ssim64"]) <= 1e-12, name
        worst = max(worst, abs(float(golden[name + "__ssim64"] - golden[name + "__ssim"])))
    assert 1e-8 < worst < 1e-5


def test_recorded_reference_values_are_what_the_issue_names(golden):
    assert golden["constant_77__ssim"] == 1.0 and golden["constant_77__mse"] == 0.0 and np.isinf(golden["constant_77__psnr"])
    assert abs(float(golden["black_on_white__ssim"]) - 9.999e-5) < 1e-8 and golden["black_on_white__mse"] == 1.0
    assert golden["inverse__ssim"] < -0.9   # negative covariance


def test_oracle_equals_the_reference_functions_where_the_checkout_exists(golden, cases):
    if not os.path.exists(os.path.join(REFERENCE, "wildgaussians", "evaluation.py")):
        pytest.skip("reference checkout not present")
    ns = L.reference_functions(REFERENCE)
    for name, (c, pred, gt, o) in cases.items():
        v = L.reference_values(ns, c, pred, gt)
        for k in ("psnr", "ssim", "mae", "mse", "ssim64"):
            assert np.array_equal(np.asarray(v[k], np.float64), golden[f"{name}__{k}"]), (name, k)
        assert np.all(np.abs(o["ssim"] - np.asarray(v["ssim"], np.float64)) <= 1e-12), name
    edge = L.edge_floats()
    clamped = torch.clamp(torch.from_numpy(edge.copy()), 0, 1).nan_to_num_(0).numpy()
    assert np.array_equal(ns["convert_image_dtype"](clamped, np.uint8), golden["edge_bytes"])


def test_restated_quantisation_reproduces_the_recorded_bytes(golden):
    edge = L.edge_floats()
    assert np.array_equal(L.quantize(L.clamp_render(edge)), golden["edge_bytes"])
    assert set(golden["edge_bytes"].tolist()) == set(range(256))
    # truncation, not rounding: the float just under k / 255 gives k - 1
    below = np.nextafter(np.float32(128) / np.float32(255), np.float32(0))
    assert L.quantize(np.array([below], np.float32))[0] == 127


def stub_evaluation_module():
    m = types.ModuleType("stub_evaluation")
    m.calls = []

    def compute_metrics(pred, gt, *, reduce=True, run_lpips_vgg=False):
        m.calls.append((pred, gt, reduce, run_lpips_vgg))
        return {"original": True}

    m.compute_metrics = compute_metrics
    m.lpips = lambda a, b: np.full(a.shape[:-3], 0.25)
    m.lpips_vgg = lambda a, b: np.full(a.shape[:-3], 0.5)
    return m


def test_fuse_evaluation_metrics_swaps_only_when_called_and_undoes():
    import wg_integration
    m = stub_evaluation_module()
    original = m.compute_metrics
    assert m.compute_metrics is original                      # importing wg_integration swaps nothing
    undo = wg_integration.fuse_evaluation_metrics(m)
    assert m.compute_metrics is not original
    f64 = np.zeros((16, 16, 3), np.float64)
    small = np.zeros((10, 16, 3), np.uint8)
    u8 = np.zeros((16, 16, 3), np.uint8)
    five = np.zeros((16, 16, 5), np.uint8)
    for pred, gt, kw in ((f64, f64, {}), (small, small, {"reduce": False}), ("not an array", u8, {}), (u8, [[1]], {"run_lpips_vgg": True}),
                         (five, five, {}), (u8, np.zeros((12, 16, 3), np.uint8), {})):
        m.calls.clear()
        assert m.compute_metrics(pred, gt, **kw) == {"original": True}
        assert len(m.calls) == 1
        p, g, reduce, vgg = m.calls[0]
        assert p is pred and g is gt and reduce == kw.get("reduce", True) and vgg == kw.get("run_lpips_vgg", False)
    undo()
    assert m.compute_metrics is original
    undo()   # a second undo changes nothing
    assert m.compute_metrics is original


def test_without_a_device_covered_calls_reach_the_original(monkeypatch):
    import wg_integration
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = stub_evaluation_module()
    undo = wg_integration.fuse_evaluation_metrics(m)
    u8 = np.zeros((16, 16, 3), np.uint8)
    assert m.compute_metrics(u8, u8) == {"original": True} and m.calls[0][0] is u8
    undo()


def test_apply_optins_signature_is_unchanged():
    import wg_integration
    names = list(inspect.signature(wg_integration.apply_optins).parameters)
    assert names[-1] == "uncertainty_metrics" and not any("evaluation" in n or "metric" in n for n in names[:-1])
    assert list(inspect.signature(wg_integration.fuse_evaluation_metrics).parameters) == ["evaluation_module"]


# =============================================================================================== GPU
def check_against_oracle(got, o):
    assert abs(got["ssim"] - float(o["ssim"])) <= SSIM_ABS, (got["ssim"], float(o["ssim"]))
    for k in ("mse", "mae"):
        want = float(o[k])
        if want == 0.0:
            assert got[k] == 0.0
        else:
            assert abs(got[k] - want) <= SUM_REL * want, (k, got[k], want)
    if got["mse"] == 0.0:
        assert got["psnr"] == math.inf
    else:
        assert got["psnr"] == -10.0 * math.log10(got["mse"])
    assert all(type(got[k]) is float for k in ("psnr", "ssim", "mae", "mse"))


def device_pred(c, pred):
    return torch.from_numpy(pred).to(DEV) if c["kind"] == "render" else pred


@gpu
@pytest.mark.parametrize("name", SINGLE)
def test_frame_metrics_against_the_oracle(cases, name):
    from wg_fused_metrics import frame_metrics
    c, pred, gt, o = cases[name]
    got = frame_metrics(device_pred(c, pred), gt, roi=c["roi"])
    print(name, {k: got[k] - float(o[k]) for k in ("ssim", "mse", "mae")})
    check_against_oracle(got, o)
    again = frame_metrics(device_pred(c, pred), gt, roi=c["roi"])
    assert same_result_bits(got, again)


@gpu
def test_tensor_inputs_and_device_resident_ground_truth(cases):
    from wg_fused_metrics import frame_metrics
    c, pred, gt, o = cases["ragged_pm6"]
    host = frame_metrics(pred, gt)
    dev = frame_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    cpu_tensor = frame_metrics(torch.from_numpy(pred), torch.from_numpy(gt))
    assert same_result_bits(host, dev) and same_result_bits(host, cpu_tensor)


@gpu
def test_a_crop_has_the_bits_of_its_contiguous_copy(cases):
    from wg_fused_metrics import frame_metrics
    c, pred, gt, o = cases["right_half"]
    y0, y1, x0, x1 = c["roi"]
    assert (x0 * gt.shape[-1]) % 4 != 0   # the crop starts at an unaligned byte
    cropped = frame_metrics(pred, gt, roi=c["roi"])
    copies = frame_metrics(np.ascontiguousarray(pred[y0:y1, x0:x1]), np.ascontiguousarray(gt[y0:y1, x0:x1]))
    assert same_result_bits(cropped, copies)
    check_against_oracle(cropped, o)


@gpu
def test_a_raw_render_has_the_bits_of_quantize_then_uint8(cases):
    from wg_fused_metrics import frame_metrics, quantize_frame
    c, pred, gt, o = cases["render"]
    render = torch.from_numpy(pred).to(DEV)
    q = quantize_frame(render)
    assert q.dtype == torch.uint8 and tuple(q.shape) == gt.shape
    assert np.array_equal(q.cpu().numpy(), L.quantize_render(pred))
    assert same_result_bits(frame_metrics(render, gt), frame_metrics(q, gt))
    # a non-contiguous render (a view of a wider frame) reads through its strides
    wide = torch.zeros((3, 43, 80), device=DEV)
    wide[:, :, :75] = render
    assert same_result_bits(frame_metrics(wide[:, :, :75], gt), frame_metrics(q, gt))


@gpu
def test_four_channel_float_prediction_against_three_channel_uint8(cases):
    from wg_fused_metrics import frame_metrics
    rng = np.random.default_rng(21)
    pred = rng.uniform(-0.2, 1.2, (20, 33, 4)).astype(np.float32)
    gt = rng.integers(0, 256, (20, 33, 3), dtype=np.uint8)
    c = dict(kind="float", roi=None)
    check_against_oracle(frame_metrics(pred, gt), L.oracle(c, pred, gt))


@gpu
def test_compute_metrics_over_a_batch(cases):
    from wg_fused_metrics import compute_metrics, frame_metrics
    c, pred, gt, o = cases["batch"]
    seen = []

    def lpips(a, b):
        seen.append((a, b))
        return np.array([0.25, 0.75], np.float32)

    full = compute_metrics(pred, gt, reduce=False, run_lpips_vgg=True, lpips=lpips, lpips_vgg=lambda a, b: np.array([1.0, 3.0]))
    assert set(full) == {"psnr", "ssim", "mae", "mse", "lpips", "lpips_vgg"}
    for k in ("psnr", "ssim", "mae", "mse"):
        assert full[k].dtype == np.float64 and full[k].shape == (2,)
    for i in range(2):
        one = frame_metrics(pred[i], gt[i])
        check_against_oracle(one, {k: o[k][i] for k in o})
        assert all(dbits(full[k][i]) == dbits(one[k]) for k in one)
    a, b = seen[0]   # the reference hands its LPIPS (gt, pred) as float32 images
    assert a.dtype == np.float32 and np.array_equal(a, gt.astype(np.float32) / 255.0) and np.array_equal(b, pred.astype(np.float32) / 255.0)
    mean = compute_metrics(pred, gt, lpips=lpips)
    assert set(mean) == {"psnr", "ssim", "mae", "mse", "lpips"} and all(type(v) is float for v in mean.values())
    assert mean["ssim"] == full["ssim"].mean().item() and mean["psnr"] == full["psnr"].mean().item() and mean["lpips"] == 0.5
    assert "lpips" not in compute_metrics(pred, gt)
    with pytest.raises(ValueError):
        compute_metrics(pred, gt, run_lpips_vgg=True)


@gpu
def test_fuse_evaluation_metrics_takes_the_fused_path_with_the_callers_lpips(cases):
    import wg_integration
    c, pred, gt, o = cases["four_against_three"]
    m = stub_evaluation_module()
    undo = wg_integration.fuse_evaluation_metrics(m)
    m.lpips = lambda a, b: np.float32(0.125)   # replaced AFTER the swap: looked up at call time
    got = m.compute_metrics(pred, gt)
    assert not m.calls and got["lpips"] == 0.125 and "lpips_vgg" not in got
    check_against_oracle({k: got[k] for k in ("psnr", "ssim", "mae", "mse")}, o)
    assert m.compute_metrics(pred, gt, run_lpips_vgg=True)["lpips_vgg"] == 0.5
    undo()
    assert m.compute_metrics(pred, gt) == {"original": True}


@gpu
def test_shapes_that_do_not_fit_raise():
    from wg_fused_metrics import frame_metrics, quantize_frame
    u8 = np.zeros((16, 16, 3), np.uint8)
    for pred, gt, roi in ((np.zeros((16, 17, 3), np.uint8), u8, None), (np.zeros((16, 16, 2), np.uint8), u8, None),
                          (np.zeros((10, 16, 3), np.uint8), np.zeros((10, 16, 3), np.uint8), None), (u8, u8, (0, 10, 0, 16)),
                          (u8, u8, (0, 17, 0, 16)), (u8, u8, (4, 15, 6, 16)), (u8.astype(np.float64), u8, None),
                          (np.zeros((16, 16, 5), np.uint8), np.zeros((16, 16, 5), np.uint8), None), (u8[0], u8, None),
                          (torch.zeros((3, 16, 16)), u8, None)):
        with pytest.raises(ValueError):
            frame_metrics(pred, gt, roi=roi)
    with pytest.raises(ValueError):
        quantize_frame(torch.zeros((5, 4, 4), device=DEV))
    with pytest.raises(ValueError):
        quantize_frame(torch.zeros((3, 4, 4)))


def desc(M, t, kind, strides):
    return M._Desc(t.data_ptr(), kind, 0, *strides)


@gpu
def test_c_abi_guards_and_refusals(cases):
    """Guard words around the scratch and the three outputs stay untouched; a rectangle under 11 x 11 and other bad arguments are refused
    before any device work."""
    import wg_fused_metrics as M
    c, pred, gt, o = cases["many_partials"]   # 10 x 19 x 3 = 570 partials: more than the finishing workgroup has threads
    H, W, ch = gt.shape
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    words = M._lib.wg_image_metrics_scratch_bytes(ch, H, W) // 8
    assert words == 3 * 10 * 19 * 3 and words // 3 > 256
    guard = -1.2345e300
    buf = torch.full((4 + 3 + 4 + words + 4,), guard, device=DEV, dtype=torch.float64)
    out_ptr, scratch_ptr = buf.data_ptr() + 32, buf.data_ptr() + 8 * 11
    a, b = desc(M, p, M.KIND_U8, p.stride()), desc(M, g, M.KIND_U8, g.stride())
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda *rect, pa=a, out=out_ptr, C_=ch: M._lib.wg_image_metrics(  # noqa: E731
        C.byref(pa), C.byref(b), H, W, C_, *rect, M._TAPS_C, M._C1, M._C2, scratch_ptr, out, stream)
    assert call(0, H, 0, W) == 0
    host = buf.cpu().numpy()
    assert np.all(host[:4] == guard) and np.all(host[7:11] == guard) and np.all(host[-4:] == guard)
    assert not np.any(host[11:-4] == guard)   # every partial was written
    check_against_oracle({"mse": float(host[4]), "mae": float(host[5]), "ssim": float(host[6]),
                          "psnr": -10.0 * math.log10(float(host[4]))}, o)
    buf.fill_(guard)
    torch.cuda.synchronize()
    for rect in ((0, 10, 0, W), (0, H, 5, 15), (0, H + 1, 0, W), (-1, H, 0, W), (20, 20, 0, W), (0, H, W - 5, W + 6)):
        assert call(*rect) == -1, rect
    assert call(0, H, 0, W, C_=5) == -1 and call(0, H, 0, W, C_=0) == -1
    assert call(0, H, 0, W, pa=desc(M, p, 3, p.stride())) == -1                       # an unknown kind
    assert call(0, H, 0, W, pa=desc(M, p, M.KIND_U8, (-1, 3, 1))) == -1                # a negative stride
    assert call(0, H, 0, W, out=out_ptr + 4) == -1                                    # a misaligned output
    assert M._lib.wg_image_metrics_scratch_bytes(3, 10, 64) == 0 and M._lib.wg_image_metrics_scratch_bytes(5, 64, 64) == 0
    torch.cuda.synchronize()
    assert bool((buf == guard).all())   # refused calls wrote nothing


QUANT_SHAPES = [(1, 1, 1), (3, 1, 2), (4, 1, 3), (3, 2, 2), (1, 5, 5), (3, 5, 5), (3, 6, 7), (4, 7, 9), (3, 8, 16), (1, 8, 16), (4, 8, 16),
                (2, 3, 5), (3, 43, 42)]   # HW % 4 = 0..3, frames smaller than a thread's four pixels, C = 1..4, more than one workgroup


@gpu
@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantize_frame_bits(golden, shape):
    from wg_fused_metrics import quantize_frame
    edge = L.edge_floats()
    n = int(np.prod(shape))
    idx = (np.arange(n) * 7 + shape[0]) % edge.size if n < edge.size else np.arange(n) % edge.size
    if n >= edge.size:
        assert len(set(idx.tolist())) == edge.size   # every edge value is in the frame
    x = edge[idx].reshape(shape)
    got = quantize_frame(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == (shape[1], shape[2], shape[0]) and got.dtype == np.uint8
    assert np.array_equal(got, np.moveaxis(golden["edge_bytes"][idx].reshape(shape), 0, -1))         # the reference's recorded bytes
    with np.errstate(invalid="ignore"):
        clamped = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1)))
        mine = np.clip(clamped * 255.0, 0, 255).astype(np.uint8)                                       # the NumPy expression, here
    assert np.array_equal(got, np.moveaxis(mine, 0, -1))


@gpu
def test_quantize_every_edge_value_and_guard_bytes(golden):
    """All 1806 edge floats through both store forms (HW % 4 == 0 with aligned addresses; an odd output address), with guard bytes around
    the output."""
    import wg_fused_metrics as M
    edge = L.edge_floats()
    stream = torch.cuda.current_stream().cuda_stream
    for HW, C_, shift in ((edge.size // 4 * 4, 1, 0), (edge.size, 1, 0), (600, 3, 0), (600, 3, 1), (451, 4, 0), (452, 4, 3)):
        n = HW * C_
        idx = np.arange(n) % edge.size
        src = torch.from_numpy(edge[idx]).to(DEV)
        dst = torch.full((16 + n + 16,), 0xA5, device=DEV, dtype=torch.uint8)
        assert M._lib.wg_frame_quantize(C_, HW, src.data_ptr(), dst.data_ptr() + 16 + shift, stream) == 0
        host = dst.cpu().numpy()
        want = np.ascontiguousarray(golden["edge_bytes"][idx].reshape(C_, HW).T).reshape(-1)
        assert np.array_equal(host[16 + shift:16 + shift + n], want), (HW, C_, shift)
        assert np.all(host[:16 + shift] == 0xA5) and np.all(host[16 + shift + n:] == 0xA5), (HW, C_, shift)
    src = torch.zeros(16, device=DEV)
    dst = torch.zeros(16, device=DEV, dtype=torch.uint8)
    assert M._lib.wg_frame_quantize(5, 3, src.data_ptr(), dst.data_ptr(), stream) == -1
    assert M._lib.wg_frame_quantize(3, 0, src.data_ptr(), dst.data_ptr(), stream) == -1
    assert M._lib.wg_frame_quantize(3, 4, None, dst.data_ptr(), stream) == -1
