"""Shared pieces of tests/test_image_metrics.py, tests/golden/make_image_metrics_golden.py and scripts/bench_image_metrics.py: the case table,
the inputs (regenerated from seeds), a NumPy restatement of the reference's evaluation chain in its operation order and dtypes
(wildgaussians/evaluation.py:156-248, utils.py:108-117, the clamp of method.py's render()), and the loader of the reference's own functions
where a checkout lies.

The chain, per image pair: uint8 -> astype(float32) / 255.0; clip to [0, 1] in float32; MSE / MAE = np.mean over float32 (a - b)^2 / |a - b|;
SSIM = dm_pix's over an 11-tap Gaussian whose taps are float64, so np.convolve promotes: float32 inputs and float32 products a*a, b*b, a*b,
float64 filtering and everything after it."""
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_metrics_ref.npz")
WINDOW = 11

# kind: how make_inputs builds the pair.  roi: (y0, y1, x0, x1) or None.  All uint8 [H, W, C] unless the kind says otherwise.
CASES = [
    dict(name="one_window", kind="noise", shape=(11, 11, 3), seed=1, roi=None),
    dict(name="one_row_of_windows", kind="noise", shape=(11, 64, 1), seed=2, roi=None),
    dict(name="one_column_of_windows", kind="noise", shape=(64, 11, 1), seed=3, roi=None),
    dict(name="ragged_pm6", kind="pm6", shape=(43, 75, 3), seed=4, roi=None),
    dict(name="constant_77", kind="constant", shape=(43, 75, 3), seed=5, roi=None),
    dict(name="inverse", kind="inverse", shape=(43, 75, 3), seed=6, roi=None),
    dict(name="black_on_white", kind="extremes", shape=(43, 75, 3), seed=7, roi=None),
    dict(name="step_edge", kind="step", shape=(43, 75, 3), seed=8, roi=None),
    dict(name="right_half", kind="noise", shape=(64, 99, 3), seed=9, roi=(0, 64, 49, 99)),
    dict(name="four_against_three", kind="pred4", shape=(43, 75, 3), seed=10, roi=None),
    dict(name="float_clip", kind="float", shape=(43, 75, 3), seed=11, roi=None),
    dict(name="render", kind="render", shape=(43, 75, 3), seed=12, roi=None),
    dict(name="many_partials", kind="pm6", shape=(300, 300, 3), seed=13, roi=None),
    dict(name="batch", kind="batch", shape=(2, 24, 37, 3), seed=14, roi=None),
]
CASE_NAMES = [c["name"] for c in CASES]


def case(name):
    return CASES[CASE_NAMES.index(name)]


def make_inputs(c):
    """-> (pred, gt).  "render": pred is a float32 [3, H, W] raw render; "pred4": pred has 4 channels; "batch": [2, H, W, C]."""
    rng = np.random.default_rng(c["seed"])
    shape, kind = tuple(c["shape"]), c["kind"]
    noise = lambda: rng.integers(0, 256, shape, dtype=np.uint8)  # noqa: E731
    if kind in ("noise", "batch"):
        return noise(), noise()
    if kind == "pm6":
        # a smooth ramp with noise on it, so that SSIM is neither 0 nor 1
        y, x, ch = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
        gt = ((y * 3 + x * 2 + ch * 40) % 200 + 20 + rng.integers(0, 16, shape)).astype(np.int64)
        pred = np.clip(gt + rng.integers(-6, 7, shape), 0, 255)
        return pred.astype(np.uint8), gt.astype(np.uint8)
    if kind == "constant":
        return np.full(shape, 77, np.uint8), np.full(shape, 77, np.uint8)
    if kind == "inverse":
        gt = noise()
        return (255 - gt).astype(np.uint8), gt
    if kind == "extremes":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    if kind == "step":
        gt = np.full(shape, 200, np.uint8)
        gt[14:24, 30:50] = 10
        pred = np.full(shape, 200, np.uint8)
        pred[15:25, 32:52] = 10   # the same block, moved by (1, 2)
        return pred, gt
    if kind == "pred4":
        gt = noise()
        pred = rng.integers(0, 256, shape[:2] + (4,), dtype=np.uint8)
        return pred, gt
    if kind == "float":
        return (rng.uniform(-0.3, 1.3, shape).astype(np.float32), rng.uniform(-0.3, 1.3, shape).astype(np.float32))
    if kind == "render":
        H, W, ch = shape
        pred = rng.uniform(-0.2, 1.2, (ch, H, W)).astype(np.float32)
        flat = pred.reshape(-1)
        special = np.array([np.nan, np.inf, -np.inf, -0.0, -1.0, 2.0, 1.0, 0.0], np.float32)
        flat[rng.choice(flat.size, 8 * special.size, replace=False)] = np.tile(special, 8)
        return pred, noise()
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------- the restated chain
def clamp_render(x):
    """torch.clamp(x, 0, 1).nan_to_num_(0) of the reference's render(), in NumPy, float32."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)


def quantize(x):
    """float32 in [0, 1] -> uint8, as convert_image_dtype(x, np.uint8): one float32 multiplication and a truncation."""
    return np.clip(x * 255.0, 0, 255).astype(np.uint8)


def quantize_render(render):
    """A raw [C, H, W] float32 render -> the uint8 [H, W, C] image the reference compares."""
    return quantize(np.moveaxis(clamp_render(render), 0, -1))


def to_float32(image):
    """convert_image_dtype(image, np.float32) for uint8 and float32."""
    return image if image.dtype == np.float32 else image.astype(np.float32) / 255.0


def normalize(a):
    return np.clip(a, 0, 1).astype(np.float32)


def taps(kernel_size=WINDOW, sigma=1.5):
    hw = kernel_size // 2
    shift = (2 * hw - kernel_size + 1) / 2
    filt = np.exp(-0.5 * ((np.arange(kernel_size) - hw + shift) / sigma) ** 2)
    return filt / np.sum(filt)


def _valid(z, axis, filt):
    """np.convolve(row, filt, mode="valid") along `axis` of a float64 array, every row at once, the taps added in ascending order."""
    n = z.shape[axis] - filt.size + 1
    out = np.zeros(z.shape[:axis] + (n,) + z.shape[axis + 1:], np.float64)
    for k in range(filt.size):
        out += np.take(z, np.arange(k, k + n), axis=axis) * filt[filt.size - 1 - k]
    return out


def ssim_map(a, b, max_val=1.0, k1=0.01, k2=0.03):
    """dm_pix's SSIM map over [H, W, C] arrays (float32 in the chain; float64 for the all-float64 yardstick)."""
    filt = taps()
    f = lambda z: _valid(_valid(z.astype(np.float64), 1, filt), 0, filt)  # noqa: E731  (x first, then y)
    mu0, mu1 = f(a), f(b)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    sigma00 = f(a ** 2) - mu00
    sigma11 = f(b ** 2) - mu11
    sigma01 = f(a * b) - mu01
    eps = np.finfo(np.float32).eps ** 2
    sigma00 = np.maximum(eps, sigma00)
    sigma11 = np.maximum(eps, sigma11)
    sigma01 = np.sign(sigma01) * np.minimum(np.sqrt(sigma00 * sigma11), np.abs(sigma01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return ((2 * mu01 + c1) * (2 * sigma01 + c2)) / ((mu00 + mu11 + c1) * (sigma00 + sigma11 + c2))


def crop(image, roi):
    if roi is None:
        return image
    y0, y1, x0, x1 = roi
    return image[..., y0:y1, x0:x1, :]


def prepare(c, pred, gt):
    """What compute_metrics sees for a case: a render quantised, the channel slice, the crop, float32 values in [0, 1]."""
    if c["kind"] == "render":
        pred = quantize_render(pred)
    pred = pred[..., : gt.shape[-1]]
    return normalize(to_float32(crop(pred, c["roi"]))), normalize(to_float32(crop(gt, c["roi"])))


def oracle(c, pred, gt):
    """{"mse", "mae", "ssim", "psnr"} as float64 (arrays of the batch shape for a batch).  MSE and MAE are summed in FLOAT64 over the
    float32 terms: the exact mean of what NumPy's float32 np.mean approximates."""
    a, b = prepare(c, pred, gt)
    d = a - b
    mse = np.mean((d * d).astype(np.float64), (-3, -2, -1))
    mae = np.mean(np.abs(d).astype(np.float64), (-3, -2, -1))
    if a.ndim == 3:
        ssim = np.mean(ssim_map(b, a))
    else:
        ssim = np.array([np.mean(ssim_map(b[i], a[i])) for i in range(a.shape[0])])
    with np.errstate(divide="ignore"):
        psnr = -10 * np.log10(mse)
    return {"mse": mse, "mae": mae, "ssim": ssim, "psnr": psnr}


# ---------------------------------------------------------------------------------------------- quantisation edge values
def edge_floats():
    """float32 vector: for every k in 0..255 the neighbours (+-3 ulps) of the point where x * 255.0f crosses k, and the special values."""
    out = []
    for k in range(256):
        x = np.float32(k) / np.float32(255.0)
        lo = hi = x
        row = [x]
        for _ in range(3):
            lo = np.nextafter(lo, np.float32(-1.0), dtype=np.float32)
            hi = np.nextafter(hi, np.float32(2.0), dtype=np.float32)
            row += [lo, hi]
        out += sorted(row)
    tiny = np.float32(1e-40)   # a denormal
    out += [0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf, -np.inf,
            tiny, -tiny, -1.0, 2.0, 0.5, 254.999 / 255.0]
    return np.array(out, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- the reference's own functions
def reference_functions(checkout):
    """mse, mae, ssim, psnr, dmpix_ssim, convert_image_dtype executed out of the reference's files (the modules themselves need packages a
    test machine may lack)."""
    from functools import wraps
    from typing import Callable, Optional, Union, cast
    ns = {"np": np, "Union": Union, "Optional": Optional, "Callable": Callable, "cast": cast, "wraps": wraps}
    for rel, names in (("wildgaussians/utils.py", {"convert_image_dtype"}),
                       ("wildgaussians/evaluation.py", {"_wrap_metric_arbitrary_shape", "dmpix_ssim", "_normalize_input", "ssim", "mse", "_mean", "mae", "psnr"})):
        path = os.path.join(checkout, rel)
        tree = ast.parse(open(path).read())
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert {n.name for n in body} == names, (rel, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def reference_values(ns, c, pred, gt):
    """The four numbers as the reference's compute_metrics forms them (evaluation.py:339-347), and dmpix_ssim on float64 copies."""
    if c["kind"] == "render":
        import torch
        frame = torch.clamp(torch.from_numpy(pred.copy()), 0, 1).nan_to_num_(0).permute(1, 2, 0).numpy()
        pred = ns["convert_image_dtype"](frame, np.uint8)
    pred, gt = crop(pred, c["roi"]), crop(gt, c["roi"])
    pred = pred[..., : gt.shape[-1]]
    pred = ns["convert_image_dtype"](pred, np.float32)
    gt = ns["convert_image_dtype"](gt, np.float32)
    mse_ = ns["mse"](pred, gt)
    with np.errstate(divide="ignore"):
        psnr_ = ns["psnr"](mse_)
    n = ns["_normalize_input"]
    return {"psnr": psnr_, "ssim": ns["ssim"](gt, pred), "mae": ns["mae"](gt, pred), "mse": mse_,
            "ssim64": ns["dmpix_ssim"](n(gt).astype(np.float64), n(pred).astype(np.float64))}
