"""Shared by tests/test_uncertainty.py, tests/golden/make_uncertainty_golden.py and scripts/bench_uncertainty_step.py: the cases, the seeded
inputs, a stand-in backbone, a stand-in model and a PyTorch restatement of the covered case of UncertaintyModel._compute_losses
(wildgaussians/method.py:363-433 with :190-201, :267-323) that runs in whatever dtype it is asked for.  In float64 it is the tests' oracle.
The oracle takes the dropout2d channel factors as an input, and optionally the features and the ssim / msssim maps, so that a kernel under
test and the oracle can be given the very same numbers."""
import json
import math
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import msssim_lib as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uncertainty_ref.npz")
PATCH = 14
SAMPLE_TARGET = 4000     # loss_mult is recorded on a strided grid of about this many pixels (the fixture's size limit)

# The smallest shapes at which each step can go wrong (tests/test_uncertainty.py).  init: "ref" = the reference's initialisation (the clamp is
# never active), "clamp" = conv_seg.weight * 40 and bias -2.5 (both the clip_min clamp and the clamp_max(3) are active on part of the frame).
CASES = [
    {"name": "60x85-ref-init", "H": 60, "W": 85, "C": 384, "training": True, "init": "ref", "steps": 1},
    {"name": "60x85-clamp", "H": 60, "W": 85, "C": 384, "training": True, "init": "clamp", "steps": 1},
    {"name": "56x84-C20-no-pads", "H": 56, "W": 84, "C": 20, "training": True, "init": "clamp", "steps": 1},
    {"name": "366x527-down-twice", "H": 366, "W": 527, "C": 384, "training": True, "init": "clamp", "steps": 2},
    {"name": "720x400-portrait-eval", "H": 720, "W": 400, "C": 384, "training": False, "init": "clamp", "steps": 1},
    {"name": "25x360-up-and-down", "H": 25, "W": 360, "C": 20, "training": True, "init": "clamp", "steps": 1},    # -> 28x350: rows ENLARGED
    {"name": "14x700-one-axis", "H": 14, "W": 700, "C": 20, "training": True, "init": "clamp", "steps": 1},        # -> 14x350: rows unchanged
]
# Seeds chosen (by the generator's search) so that in the float64 oracle no pixel of the last step has |bilinear(s) - clip_min| < 1e-5: the
# clamp's derivative is discontinuous there, and a float32 kernel may fall on the other side.  The generator asserts the margin.
for _c, _seed in zip(CASES, (4100, 4101, 4202, 6803, 6804, 4105, 4106)):
    _c["seed"] = _seed
CONFIG = {"uncertainty_mode": "dino", "uncertainty_dino_max_size": None, "uncertainty_dropout": 0.5, "uncertainty_clip_min": 0.1,
          "uncertainty_regularizer_weight": 0.5}   # the reference's defaults (config.py:77-85)
RESULT_NAMES = ("loss", "ssim", "msssim", "ssim_discounted", "mse_discounted", "psnr_discounted", "beta")
TENSORS = ("s", "loss_mult", "result", "d_bn_weight", "d_bn_bias", "d_conv_weight", "d_conv_bias", "running_mean", "running_var")


def case_id(c):
    return c["name"]


# ---------------------------------------------------------------------------------------------- sizes
def pads(n, P=PATCH):
    d = math.ceil(n / P) * P - n
    return d // 2, d - d // 2


def down_size(H, W, max_size=350):
    if max_size < H or max_size < W:
        f = min(max_size / H, max_size / W)
        return ((int(H * f) + 13) // 14) * 14, ((int(W * f) + 13) // 14) * 14
    return H, W


def sample_stride(c):
    return max(1, math.ceil(math.sqrt(c["H"] * c["W"] / SAMPLE_TARGET)))


# ---------------------------------------------------------------------------------------------- inputs
def make_images(c, step=0):
    """float32 CPU gt, prediction [1, 3, H, W] of case `c` (and of its step-th call), from its seed alone: a smooth image plus fine noise, and
    a prediction that is close to it in some regions and far from it in others, so that the cosine term covers both ends of its clip."""
    g = torch.Generator().manual_seed(c["seed"] * 10 + step)
    H, W = c["H"], c["W"]
    low = torch.rand((1, 3, H // 8 + 2, W // 8 + 2), generator=g)
    gt = (F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False) + 0.05 * torch.randn((1, 3, H, W), generator=g)).clamp(0, 1)
    mask = F.interpolate(torch.rand((1, 1, H // 24 + 2, W // 24 + 2), generator=g), size=(H, W), mode="bilinear", align_corners=False) ** 2
    pred = (gt + mask * torch.randn((1, 3, H, W), generator=g)).clamp(0, 1)
    return gt.contiguous(), pred.contiguous()


class StandInBackbone(torch.nn.Module):
    """patch_size 14, embed_dim C, num_heads: get_intermediate_layers returns tanh of a seeded 14x14 stride-14 convolution.  The convolution
    is evaluated as a float64 matrix product and rounded to the input's dtype, so a float32 caller gets correctly rounded features on every
    device (the backbone is not under test)."""
    patch_size = PATCH
    num_heads = 6

    def __init__(self, C, seed):
        super().__init__()
        self.embed_dim = C
        g = torch.Generator().manual_seed(seed)
        # plain attributes, not buffers: model.to(dtype) must not round them
        self._weight = 0.03 * torch.randn((C, 3 * PATCH * PATCH), generator=g, dtype=torch.float64)
        self._bias = 0.2 * torch.randn((C,), generator=g, dtype=torch.float64)
        self._on = {}

    def _params(self, device):
        if device not in self._on:
            self._on[device] = (self._weight.t().contiguous().to(device), self._bias.to(device))
        return self._on[device]

    def get_intermediate_layers(self, x, n, reshape=True):
        assert reshape and list(n) == [self.num_heads - 1]
        B, ch, Hp, Wp = x.shape
        hp, wp = Hp // PATCH, Wp // PATCH
        cols = x.reshape(B, ch, hp, PATCH, wp, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, hp * wp, ch * PATCH * PATCH).double()
        wt, bias = self._params(x.device)
        out = torch.tanh(cols @ wt + bias)
        return (out.permute(0, 2, 1).reshape(B, self.embed_dim, hp, wp).to(x.dtype).contiguous(),)


def init_head(model, c):
    """Seeded head state of case `c` on a model with bn / conv_seg: non-trivial affine parameters and running statistics in every case."""
    g = torch.Generator().manual_seed(c["seed"] + 7)
    C = c["C"]
    with torch.no_grad():
        model.conv_seg.weight.copy_(0.01 * torch.randn((1, C, 1, 1), generator=g))   # the reference's normal_(0, 0.01)
        model.conv_seg.bias.zero_()
        if c["init"] == "clamp":
            model.conv_seg.weight.mul_(40.0)
            model.conv_seg.bias.fill_(-2.5)
        model.bn.weight.copy_(1.0 + 0.2 * torch.randn((C,), generator=g))
        model.bn.bias.copy_(0.2 * torch.randn((C,), generator=g))
        model.bn.running_mean.copy_(0.2 * torch.randn((C,), generator=g))
        model.bn.running_var.copy_(0.1 + 0.3 * torch.rand((C,), generator=g))
        model.bn.num_batches_tracked.fill_(3)


class StandInModel(torch.nn.Module):
    """The attributes wg_fused_uncertainty.compute_losses uses, built like the reference's UncertaintyModel (method.py:208-265) but with the
    stand-in backbone: config, bn, conv_seg, img_norm_mean, img_norm_std, patch_size, training, _get_dino_cached, _images_cache."""

    def __init__(self, c, config=None):
        super().__init__()
        self.config = types.SimpleNamespace(**dict(CONFIG, **(config or {})))
        self.backbone = StandInBackbone(c["C"], c["seed"] + 3)
        self.patch_size = self.backbone.patch_size
        self.conv_seg = torch.nn.Conv2d(c["C"], 1, kernel_size=1)
        self.bn = torch.nn.SyncBatchNorm(c["C"])
        self.register_buffer("img_norm_mean", torch.tensor([123.675, 116.28, 103.53], dtype=torch.float32) / 255.)
        self.register_buffer("img_norm_std", torch.tensor([58.395, 57.12, 57.375], dtype=torch.float32) / 255.)
        self._images_cache = {}
        init_head(self, c)
        self.train(c["training"])

    def _get_dino_cached(self, x, cache_entry=None):
        """As the reference's (method.py:257-265): a miss is stored under the shape of the FEATURES, a lookup asks for the shape of the INPUT."""
        if cache_entry is None or (cache_entry, x.shape) not in self._images_cache:
            with torch.no_grad():
                x = self.backbone.get_intermediate_layers(x, n=[self.backbone.num_heads - 1], reshape=True)[-1]
            if cache_entry is not None:
                self._images_cache[(cache_entry, x.shape)] = x.detach().cpu()
        else:
            x = self._images_cache[(cache_entry, x.shape)].to(x.device)
        return x


class InputKeyedModel(StandInModel):
    """A model whose cache is keyed by the shape of the input on both sides, so that a second call with the same entry is a hit."""

    def _get_dino_cached(self, x, cache_entry=None):
        key = (cache_entry, x.shape)
        if cache_entry is None or key not in self._images_cache:
            with torch.no_grad():
                x = self.backbone.get_intermediate_layers(x, n=[self.backbone.num_heads - 1], reshape=True)[-1]
            if cache_entry is not None:
                self._images_cache[key] = x.detach().cpu()
        else:
            x = self._images_cache[key].to(x.device)
        return x


# ---------------------------------------------------------------------------------------------- the oracle
def prep(img, mean, std, h, w, P=PATCH):
    """Zero padding to multiples of P of (bilinear(img -> h x w) - mean) / std; no resize at the image's own size."""
    if tuple(img.shape[2:]) != (h, w):
        img = F.interpolate(img, size=(h, w), mode="bilinear", align_corners=False)
    x = (img - mean.to(img)[None, :, None, None]) / std.to(img)[None, :, None, None]
    (pt, pb), (pl, pr) = pads(h, P), pads(w, P)
    return F.pad(x, (pl, pr, pt, pb))


def down(t):
    nh, nw = down_size(*t.shape[2:])
    return t if (nh, nw) == tuple(t.shape[2:]) else F.interpolate(t, size=(nh, nw), mode="bilinear", align_corners=False)


def oracle_features(backbone, mean, std, gt, pred):
    """-> (feat(gt) at H x W, feat(down(gt)), feat(down(pred))), each [1, C, h, w] in the images' dtype."""
    H, W = gt.shape[2:]
    nh, nw = down_size(H, W)
    f = lambda img, h, w: backbone.get_intermediate_layers(prep(img, mean, std, h, w), n=[backbone.num_heads - 1], reshape=True)[-1]
    return f(gt, H, W), f(gt, nh, nw), f(pred, nh, nw)


def oracle(head, config, training, gt, pred, kdrop, feats, ssim_map=None, msssim_map=None):
    """The covered case in the dtype of `gt`.  head: dict of bn_weight, bn_bias, conv_weight [C], conv_bias [1], running_mean, running_var, eps,
    momentum (tensors are cast to the dtype; nothing is modified).  kdrop [C]: the dropout2d channel factors.  feats: oracle_features(...).
    ssim_map / msssim_map [H, W]: the two metric maps (computed here by tests/msssim_lib.py when None).
    -> dict of TENSORS (numpy), plus `clamp_margin` = min |bilinear(s) - clip_min| over the cropped frame and the clamp fractions."""
    dt = gt.dtype
    H, W = gt.shape[2:]
    x, f_gt, f_pred = (t.to(dt) for t in feats)
    C, hp, wp = x.shape[1:]
    N = hp * wp
    gamma, beta, w, b = (head[k].detach().to(dt).reshape(-1).clone().requires_grad_(True) for k in ("bn_weight", "bn_bias", "conv_weight", "conv_bias"))
    rm, rv = head["running_mean"].detach().to(dt), head["running_var"].detach().to(dt)
    k = kdrop.to(dt).reshape(1, C, 1, 1)
    xk = x * k
    if training:
        m = xk.mean((0, 2, 3))
        v = xk.var((0, 2, 3), unbiased=False)
        mom = head["momentum"]
        rm, rv = (1 - mom) * rm + mom * m, (1 - mom) * rv + mom * v * (N / (N - 1))
    else:
        m, v = rm, rv
    xh = (xk - m.reshape(1, C, 1, 1)) / torch.sqrt(v.reshape(1, C, 1, 1) + head["eps"])
    logit = (w.reshape(1, C, 1, 1) * (gamma.reshape(1, C, 1, 1) * xh + beta.reshape(1, C, 1, 1))).sum(1, keepdim=True) + b + math.log(math.e - 1)
    s = F.softplus(logit)
    (pt, _), (pl, _) = pads(H), pads(W)
    bil = F.interpolate(s, size=(hp * PATCH, wp * PATCH), mode="bilinear", align_corners=False)[:, :, pt:pt + H, pl:pl + W]
    clip_min = config["uncertainty_clip_min"]
    u = bil.clamp(min=clip_min)
    lm = 1 / (2 * u * u)
    beta_term = torch.log(u).mean()
    # the DINO part on the downsampled grid
    nh, nw = down_size(H, W)
    (dpt, _), (dpl, _) = pads(nh), pads(nw)
    cos = F.cosine_similarity(f_gt, f_pred, dim=1).unsqueeze(1)
    cos = F.interpolate(cos, size=(cos.shape[2] * PATCH, cos.shape[3] * PATCH), mode="bilinear", align_corners=False)[:, :, dpt:dpt + nh, dpl:dpl + nw]
    dino_part = (1 - (cos - 0.5) / 0.5).clamp(0, 1).detach()
    uloss = (dino_part * down(lm)).mean()
    loss = uloss + config["uncertainty_regularizer_weight"] * beta_term
    dg, dbeta, dw, db = torch.autograd.grad(loss, (gamma, beta, w, b))
    loss_mult = lm.detach().clamp(max=3)
    if ssim_map is None:
        ssim_map = M.ref_ssim_down(gt, pred, max_size=400)[0]
        msssim_map = M.ref_msssim(gt, pred, max_size=400, min_size=80)[0]
    ss, ms = ssim_map.to(dt).reshape(1, 1, H, W), msssim_map.to(dt).reshape(1, 1, H, W)
    mse = (gt - pred) ** 2
    mse_d = (mse * loss_mult).sum() / loss_mult.sum()
    result = torch.stack([loss.detach(), ss.mean(), ms.mean(), (ss * loss_mult).sum() / loss_mult.sum(), mse_d, 10 * torch.log10(1 / mse_d),
                          beta_term.detach(), uloss.detach()])
    out = {"s": s.detach()[0, 0], "loss_mult": loss_mult[0, 0], "result": result, "d_bn_weight": dg, "d_bn_bias": dbeta, "d_conv_weight": dw,
           "d_conv_bias": db, "running_mean": rm, "running_var": rv, "dino_part": dino_part[0, 0]}
    out = {n: t.numpy() for n, t in out.items()}
    out["clamp_margin"] = float((bil.detach() - clip_min).abs().min())
    out["frac_clip_min"] = float((bil.detach() <= clip_min).double().mean())
    out["frac_clamp_max"] = float((lm.detach() >= 3).double().mean())
    return out


def head_state(model):
    return {"bn_weight": model.bn.weight, "bn_bias": model.bn.bias, "conv_weight": model.conv_seg.weight, "conv_bias": model.conv_seg.bias,
            "running_mean": model.bn.running_mean, "running_var": model.bn.running_var, "eps": model.bn.eps, "momentum": model.bn.momentum}


def run_oracle_case(c, kdrops, dtype=torch.float64):
    """Case `c` (all of its steps; the running statistics carry over) through the oracle on the CPU with the dropout factors kdrops[step]
    -> the last step's outputs."""
    model = StandInModel(c)
    head = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in head_state(model).items()}
    out = None
    for step in range(c["steps"]):
        gt, pred = (t.to(dtype) for t in make_images(c, step))
        feats = oracle_features(model.backbone, model.img_norm_mean, model.img_norm_std, gt, pred)
        out = oracle(head, CONFIG, c["training"], gt, pred, torch.as_tensor(kdrops[step]), feats)
        head["running_mean"], head["running_var"] = torch.from_numpy(out["running_mean"]), torch.from_numpy(out["running_var"])
    return out


def load_golden():
    """-> list of (case, arrays): arrays[name] for name in f"{tensor}32" / f"{tensor}64" (loss_mult on the strided grid), "kdrop" [steps, C],
    "ref32_dev" {tensor: float}, "metrics32" / "metrics64" {name: float}, "cache" [[key shape...]]."""
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    meta = json.loads(str(z["meta"]))
    out = []
    for i, c in enumerate(cases):
        arrays = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        arrays.update(meta[i])
        out.append((c, arrays))
    return out
