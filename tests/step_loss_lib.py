"""Oracle and cases of the fused train-step image loss (wg_fused_ssim.step_loss; include/wg_step_loss.h).

`statements` restates, in PyTorch and in the dtype of its inputs, the reference's train step between the render and the end of its logging
block (wildgaussians/method.py:1920-1992, uncertainty_scale_grad and uncertainty_center_mult off): scale_grads by the mask, the multiplier's
threshold and warm-up blend, the L1 and SSIM terms, the loss, its backward pass, and every logged metric.  Run in float64 it is the oracle;
tests/golden/step_loss_ref.npz, recorded from the reference's own statements (tests/golden/make_step_loss_golden.py), pins it to 1e-12.  Run in
float32 it is the reference's own float32 result for shapes the fixture does not store.
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_loss_ref.npz")

# The stats vector's entries in order (include/wg_step_loss.h: enum wg_step_stat).
STATS = ("loss", "l1_loss", "ssim", "mse", "psnr", "l1_weighted", "dssim_weighted", "mask_percentage", "ssim_masked", "mse_masked", "psnr_masked",
         "l1_loss_masked")
LOGGED = ("l1_loss", "ssim", "mse", "loss", "psnr")
LOGGED_MASKED = ("mask_percentage", "ssim_masked", "mse_masked", "psnr_masked", "l1_loss_masked")
LAMBDA = 0.2

# The recorded cases.  `schedule` = (iteration, uncertainty_warmup_start, uncertainty_warmup_iters) or None (no uncertainty model): before,
# during (p = 0.375) and after the warm-up.  Frames of at most 45 x 70 keep the fixture small.
CASES = [
    {"name": "plain_3x45x70", "shape": (3, 45, 70), "mask": "none", "schedule": None, "seed": 1},
    {"name": "binary_mask_3x23x37", "shape": (3, 23, 37), "mask": "binary", "schedule": None, "seed": 2},
    {"name": "fractional_mask_before_warmup_3x19x31", "shape": (3, 19, 31), "mask": "fractional", "schedule": (500, 1000, 800), "seed": 3},
    {"name": "binary_mask_during_warmup_3x24x33", "shape": (3, 24, 33), "mask": "binary", "schedule": (1300, 1000, 800), "seed": 4},
    {"name": "no_mask_after_warmup_3x21x29", "shape": (3, 21, 29), "mask": "none", "schedule": (5000, 1000, 800), "seed": 5},
    {"name": "binary_mask_after_warmup_1x33x47", "shape": (1, 33, 47), "mask": "binary", "schedule": (5000, 1000, 800), "seed": 6},
]


def blend_of(schedule):
    """method.py:1936-1940 as the operator's mult_blend: 0 before the warm-up, p during it, 1 after it."""
    it, start, iters = schedule
    if it < start:
        return 0.0
    if it < start + iters:
        return (it - start) / iters
    return 1.0


def make_mask(kind, H, W, g):
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(1, H, W)
    if kind == "zeros":
        return torch.zeros(1, H, W)
    if kind == "binary":
        return (torch.rand(1, H, W, generator=g) < 0.7).float()
    if kind == "fractional":   # an 8-bit mask image divided by 255
        return torch.randint(0, 256, (1, H, W), generator=g).float() / 255.0
    raise ValueError(kind)


def make_raw_mult(H, W, g):
    """A raw multiplier as the uncertainty model returns it: values on both sides of 1, some exactly 1.0, one NaN (where the frame has room)."""
    m = torch.rand(1, H, W, generator=g) * 2.0
    flat = m.view(-1)
    flat[::7] = 1.0
    if flat.numel() > 3:
        flat[3] = float("nan")
    return m


def make_inputs(shape, mask_kind, with_mult, seed):
    """float32 CPU tensors: toned, raw, gt [C, H, W]; mask, mult [1, H, W] or None."""
    Cn, H, W = shape
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    toned = gt * 0.6 + 0.4 * torch.rand(shape, generator=g)
    raw = gt * 0.5 + 0.5 * torch.rand(shape, generator=g)
    mask = make_mask(mask_kind, H, W, g)
    mult = make_raw_mult(H, W, g) if with_mult else None
    return toned, raw, gt, mask, mult


def scale_grads(values, scale):
    """method.py:120-123, restated."""
    grad_values = values * scale
    rest_values = values.detach() * (1 - scale)
    return grad_values + rest_values


def ssim(img1, img2, window_size=11, size_average=True):
    """method.py:644-673, restated (as tests/test_ssim.py's ref_ssim)."""
    sigma = 1.5
    channel = img1.size(-3)
    gauss = torch.Tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    w1 = (gauss / gauss.sum()).unsqueeze(1)
    window = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()
    window = window.to(img1.device).type_as(img1)
    conv = lambda t: F.conv2d(t, window, padding=window_size // 2, groups=channel)  # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.mean(-3)


def _log10(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.log10(np.float64(x)))


def statements(toned, raw, gt, mask=None, mult=None, lam=LAMBDA, threshold=None, blend=1.0, one_image=False, grad_scale=1.0):
    """method.py:1920-1992 in the inputs' dtype.  mult: the raw multiplier; threshold / blend: the schedule as the operator takes it.
    one_image: `toned` feeds both terms (raw is ignored).  Returns {"stats": {name: float}, "grad_toned", "grad_raw" (None when one_image),
    "mult": the effective multiplier as a tensor or the float 1.0}."""
    image_toned = toned.detach().clone().requires_grad_(True)
    image = image_toned if one_image else raw.detach().clone().requires_grad_(True)
    leaf_toned, leaf_raw = image_toned, image
    if mask is not None:
        image = scale_grads(image, mask)
        image_toned = image if one_image else scale_grads(image_toned, mask)
    loss_mult = 1.0
    if mult is not None:
        loss_mult = mult
        if threshold is not None:
            loss_mult = (loss_mult > threshold).to(dtype=loss_mult.dtype)
        if blend == 0:
            loss_mult = 1.0
        elif blend != 1:
            loss_mult = 1 + blend * (loss_mult - 1)
    Ll1 = F.l1_loss(image_toned, gt, reduction="none")
    ssim_value = ssim(image, gt, size_average=False)
    l1_weighted, dssim_weighted = (Ll1 * loss_mult).mean(), ((1.0 - ssim_value) * loss_mult).mean()
    loss = (1.0 - lam) * l1_weighted + lam * dssim_weighted
    (loss * grad_scale).backward()
    with torch.no_grad():
        mse = (image_toned - gt).pow(2)
        s = {"loss": loss.item(), "l1_loss": Ll1.mean().item(), "ssim": ssim_value.mean().item(), "mse": mse.mean().item(),
             "l1_weighted": l1_weighted.item(), "dssim_weighted": dssim_weighted.item()}
        s["psnr"] = (20 * math.log10(1.) - 10 * torch.log10(mse.mean())).item()
        nan = float("nan")
        s.update({k: nan for k in LOGGED_MASKED})
        if mask is not None:
            reduce = lambda t: ((t * mask).sum() / mask.sum()).item()  # noqa: E731
            s["mask_percentage"] = mask.mean().item()
            s["ssim_masked"], s["mse_masked"], s["l1_loss_masked"] = reduce(ssim_value), reduce(mse), reduce(Ll1)
            s["psnr_masked"] = 20 * math.log10(1.) - 10 * _log10(s["mse_masked"])   # math.log10 of a Python float; inf / NaN instead of raising
    return {"stats": s, "grad_toned": leaf_toned.grad.detach(), "grad_raw": None if one_image else leaf_raw.grad.detach(), "mult": loss_mult}


def oracle(toned, raw, gt, mask=None, mult=None, **kw):
    """`statements` in float64 on the float32 inputs' values."""
    up = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    return statements(up(toned), up(raw), up(gt), up(mask), up(mult), **kw)


def stats_vector(s):
    return np.array([s[k] for k in STATS], dtype=np.float64)


def case_kwargs(case):
    """The operator's schedule arguments of a recorded case."""
    if case["schedule"] is None:
        return {"threshold": None, "blend": 1.0}
    return {"threshold": 1.0, "blend": blend_of(case["schedule"])}


def load_golden():
    """[(case, arrays)]: arrays has toned, raw, gt, (mask), (mult), and per precision p in ("32", "64") stats<p> (float64 vector in STATS order, NaN
    where the reference logs nothing), grad_toned<p>, grad_raw<p>."""
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    out = []
    for i, c in enumerate(cases):
        c["shape"] = tuple(c["shape"])
        c["schedule"] = None if c["schedule"] is None else tuple(c["schedule"])
        out.append((c, {k[len(f"{i}_"):]: z[k] for k in z.files if k.startswith(f"{i}_")}))
    return out
