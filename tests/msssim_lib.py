"""Shared by tests/test_msssim.py and tests/golden/make_msssim_golden.py: the cases, the seeded inputs and a PyTorch restatement of the
reference's ssim_down / _ssim_parts / msssim (wildgaussians/method.py:126-187; ssim: :644-673) that runs in whatever dtype its inputs have.
In float64 it is the tests' oracle; it keeps the reference's float32-built window (`torch.Tensor([...])`, normalised and multiplied out in
float32, then cast), as the reference itself would on float64 inputs."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msssim_ref.npz")

# fn, shape, kind, arguments.  The smallest shapes at which each step can go wrong (see tests/test_msssim.py).
CASES = [
    {"fn": "msssim", "shape": (3, 37, 53), "kind": "noise", "max_size": None, "min_size": 8},    # 37x53 -> 18x26 -> 9x13 -> 4x6
    {"fn": "msssim", "shape": (3, 37, 53), "kind": "close", "max_size": 24, "min_size": 8},      # 24x34: non-integer area windows
    {"fn": "msssim", "shape": (3, 120, 161), "kind": "noise", "max_size": 40, "min_size": 10},   # 40x53 -> 20x26 -> 10x13, x3 upsampling
    {"fn": "msssim", "shape": (3, 64, 96), "kind": "close", "max_size": None, "min_size": 200},  # one level: l*c*s alone
    {"fn": "msssim", "shape": (1, 16, 16), "kind": "noise", "max_size": None, "min_size": 8},    # one channel, one pooled level
    {"fn": "msssim", "shape": (3, 7, 5), "kind": "noise", "max_size": 24, "min_size": 8},        # smaller than the window; upsample at scale 1
    {"fn": "msssim", "shape": (2, 3, 33, 47), "kind": "close", "max_size": 24, "min_size": 8},   # batch
    {"fn": "msssim", "shape": (3, 45, 30), "kind": "flat", "max_size": 24, "min_size": 8},       # clamp before sqrt
    {"fn": "ssim_down", "shape": (3, 37, 53), "kind": "noise", "max_size": None},
    {"fn": "ssim_down", "shape": (3, 37, 53), "kind": "close", "max_size": 24},
    {"fn": "ssim_down", "shape": (3, 37, 53), "kind": "noise", "max_size": 40},                  # 40x57: a slight area UPsampling
    {"fn": "ssim_down", "shape": (3, 120, 161), "kind": "close", "max_size": None},
    {"fn": "ssim_down", "shape": (3, 120, 161), "kind": "noise", "max_size": 24},
    {"fn": "ssim_down", "shape": (3, 120, 161), "kind": "close", "max_size": 40},
    {"fn": "ssim_down", "shape": (3, 7, 5), "kind": "noise", "max_size": 24},                    # area upsampling to 33x24
    {"fn": "ssim_down", "shape": (3, 45, 30), "kind": "flat", "max_size": 24},
]
for _n, _c in enumerate(CASES):
    _c["seed"] = 1000 + _n


def case_id(c):
    return "{}-{}-{}-max{}{}".format(c["fn"], "x".join(map(str, c["shape"])), c["kind"], c["max_size"],
                                     "-min{}".format(c["min_size"]) if c["fn"] == "msssim" else "")


def make_inputs(c):
    """float32 CPU images of case `c`, from its seed alone."""
    g = torch.Generator().manual_seed(c["seed"])
    shape = tuple(c["shape"])
    if c["kind"] == "noise":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if c["kind"] == "close":
        x = torch.rand(shape, generator=g)
        return x, x + 0.05 * torch.randn(shape, generator=g)
    if c["kind"] == "flat":   # piecewise constant: 20x20 blocks (wider than the window also after the area resize), so that window variances cancel
                              # to about 0, and below 0 in float32, inside a block; y is an increasing
        H, W = shape[-2:]     # affine function of x per channel (y == x in one of them), which keeps every exact SSIM factor within (0, 1]
        a = torch.rand(shape[:-2] + ((H + 19) // 20, (W + 19) // 20), generator=g)
        x = a.repeat_interleave(20, -2).repeat_interleave(20, -1)[..., :H, :W].contiguous()
        ch = torch.arange(shape[-3]) % 3
        gain, offset = torch.tensor([0.7, 1.0, 0.4])[ch, None, None], torch.tensor([0.15, 0.0, 0.3])[ch, None, None]
        return x, x * gain + offset
    raise ValueError(c["kind"])


def call_kwargs(c):
    return {"max_size": c["max_size"], "min_size": c["min_size"]} if c["fn"] == "msssim" else {"max_size": c["max_size"]}


def _window(img):
    channel = img.size(-3)
    gauss = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w1 = (gauss / gauss.sum()).unsqueeze(1)
    window = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, 11, 11).contiguous()
    return window.to(img.device).type_as(img), channel


def _moments(img1, img2):
    window, channel = _window(img1)
    conv = lambda t: F.conv2d(t, window, padding=5, groups=channel)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    return mu1_sq, mu2_sq, mu1_mu2, conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2


def ref_ssim(img1, img2, size_average=True):
    """method.py:644-673, restated: the product form."""
    mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12 = _moments(img1, img2)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.mean(1)


def ref_ssim_parts(img1, img2):
    """method.py:138-168, restated."""
    mu1_sq, mu2_sq, mu1_mu2, s1, s2, s12 = _moments(img1, img2)
    sd1, sd2 = torch.sqrt(s1.clamp_min(0)), torch.sqrt(s2.clamp_min(0))
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    C3 = C2 / 2
    return ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1), (2 * sd1 * sd2 + C2) / (s1 + s2 + C2), (s12 + C3) / (sd1 * sd2 + C3))


def ref_msssim(x, y, max_size=None, min_size=200):
    """method.py:171-187, restated.  [B, C, H, W] -> [B, H, W]."""
    raw = x.shape[-2:]
    if max_size is not None:
        scale = min(1, max(max_size / x.shape[-2], max_size / x.shape[-1]))
        x = F.interpolate(x, scale_factor=scale, mode="area")
        y = F.interpolate(y, scale_factor=scale, mode="area")
    maps = list(ref_ssim_parts(x, y))
    size0 = x.shape[-2:]
    while x.shape[-2] > min_size and x.shape[-1] > min_size:
        x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        maps.extend(F.interpolate(m, size=size0, mode="bilinear") for m in ref_ssim_parts(x, y)[1:])
    out = torch.stack(maps, -1).prod(-1)
    if max_size is not None:
        out = F.interpolate(out, size=raw, mode="bilinear")
    return out.mean(1)


def ref_ssim_down(x, y, max_size=None):
    """method.py:126-135, restated.  [B, C, H, W] -> [B, H, W]."""
    osize = x.shape[2:]
    if max_size is not None:
        scale = max(max_size / x.shape[-2], max_size / x.shape[-1])
        x = F.interpolate(x, scale_factor=scale, mode="area")
        y = F.interpolate(y, scale_factor=scale, mode="area")
    out = ref_ssim(x, y, size_average=False).unsqueeze(1)
    if max_size is not None:
        out = F.interpolate(out, size=osize, mode="bilinear", align_corners=False)
    return out.squeeze(1)


def run_case(c, fns, dtype):
    """Case `c` through fns = {"msssim": ..., "ssim_down": ...} in `dtype` on the CPU -> an array of the case's result shape."""
    x, y = (t.to(dtype) for t in make_inputs(c))
    lead = x.dim() == 3
    if lead:
        x, y = x[None], y[None]
    out = fns[c["fn"]](x, y, **call_kwargs(c))
    return (out[0] if lead else out).numpy()


ORACLE = {"msssim": ref_msssim, "ssim_down": ref_ssim_down}


def load_golden():
    """-> list of (case, out32, out64, ref32_dev) in the order of the fixture's own case list."""
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    for c in cases:
        c["shape"] = tuple(c["shape"])
    return [(c, z[f"out32_{i}"], z[f"out64_{i}"], float(z["ref32_dev"][i])) for i, c in enumerate(cases)]
