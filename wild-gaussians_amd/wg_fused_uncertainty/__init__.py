"""Fused uncertainty head and DINO loss -- opt-in replacement of `UncertaintyModel._compute_losses` (wildgaussians/method.py:363-433) in the
reference's default mode, for everything AROUND the frozen backbone (include/wg_uncertainty.h, csrc/uncertainty/uncertainty.hip).

    from wg_fused_uncertainty import compute_losses
    loss, metrics, loss_mult = compute_losses(uncertainty_model, gt, prediction, prefix, _cache_entry=key, original=orig_method)

Covered case (anything else goes to `original`, the caller's own method): uncertainty_mode == "dino", uncertainty_dino_max_size is None, float32
`gt` / `prediction` of one shape [1, 3, H, W] on a HIP device, a prediction that does not require grad, a batch norm with affine parameters,
running statistics and a numeric momentum, a C -> 1 1x1 `conv_seg` with bias, no initialised process group.  The backbone is called through the
model's own `_get_dino_cached`, so its CPU cache keeps its keys, shapes and contents.  Gradients reach conv_seg.weight, conv_seg.bias, bn.weight
and bn.bias; the metrics come from one 8-float result vector with ONE device-to-host copy.  No atomics: a repeated call gives the same bits.

The dropout2d channel factors are drawn by `draw_dropout_factors` (F.dropout2d on ones [1, C, 1, 1]): another call than the reference's, so
the random stream may differ.  Tests replace that module attribute to hand a recorded mask over.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
for _name, _res, _args in (
        ("wg_uncertainty_prepare", _i, [_i] * 9 + [_vp] * 5),
        ("wg_uncertainty_head_stats", _i, [_i] * 3 + [_vp] * 5 + [_f, _f] + [_vp] * 5),
        ("wg_uncertainty_head_forward", _i, [_i] * 2 + [_vp] * 6),
        ("wg_uncertainty_head_backward", _i, [_i] * 2 + [_vp] * 13),
        ("wg_uncertainty_maps_scratch_floats", C.c_size_t, [_i] * 2),
        ("wg_uncertainty_maps_forward", _i, [_i] * 8 + [_f] + [_vp] * 8),
        ("wg_uncertainty_cosine", _i, [_i] * 2 + [_f] + [_vp] * 4),
        ("wg_uncertainty_dino_scratch_floats", C.c_size_t, [_i] * 2),
        ("wg_uncertainty_dino_loss", _i, [_i] * 7 + [_f, _vp] + [_i] * 6 + [_vp] * 4),
        ("wg_uncertainty_finish", _i, [_i] * 4 + [_f] + [_vp] * 4),
        ("wg_uncertainty_maps_backward", _i, [_i] * 7 + [_f, _f, _vp, _i, _i] + [_vp] * 4)):
    getattr(_lib, _name).restype = _res
    getattr(_lib, _name).argtypes = _args

RESULT_NAMES = ("loss", "ssim", "msssim", "ssim_discounted", "mse_discounted", "psnr_discounted", "beta")   # result[7]: uncertainty_loss.mean()
DINO_MAX_SIZE = 350          # method.py:386
COSINE_EPS = 1e-8            # F.cosine_similarity's default; each norm is clamped on its own


# ---------------------------------------------------------------------------------------------- host size arithmetic
def pads(n: int, patch_size: int = 14):
    """UncertaintyModel._get_pad (method.py:231-236): (before, after)."""
    d = math.ceil(n / patch_size) * patch_size - n
    return d // 2, d - d // 2


def down_size(H: int, W: int, max_size: int = DINO_MAX_SIZE):
    """The size dino_downsample (method.py:190-201) resizes H x W to; H, W itself when both sides fit.  Python doubles, as the reference."""
    if max_size < H or max_size < W:
        f = min(max_size / H, max_size / W)
        return ((int(H * f) + 13) // 14) * 14, ((int(W * f) + 13) // 14) * 14
    return H, W


class Geometry:
    """Every size of one covered call."""

    def __init__(self, H: int, W: int, patch_size: int):
        P = self.P = int(patch_size)
        self.H, self.W = int(H), int(W)
        (self.pad_top, pb), (self.pad_left, pr) = pads(H, P), pads(W, P)
        self.Hp, self.Wp = H + self.pad_top + pb, W + self.pad_left + pr
        self.hp, self.wp = self.Hp // P, self.Wp // P
        self.nh, self.nw = down_size(H, W)
        (self.dpad_top, pb), (self.dpad_left, pr) = pads(self.nh, P), pads(self.nw, P)
        self.nhp, self.nwp = self.nh + self.dpad_top + pb, self.nw + self.dpad_left + pr
        self.hd, self.wd = self.nhp // P, self.nwp // P


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need(name, *tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"wg_fused_uncertainty.{name}: float32 tensors on a HIP device are required (there is no CPU path)")


def _f32(t):
    return t.detach().contiguous()


# ---------------------------------------------------------------------------------------------- tensor-level pieces
def prepare_backbone_input(img: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, h: int, w: int, patch_size: int = 14) -> torch.Tensor:
    """[1, C, H, W] -> [1, C, hP, wP]: F.pad((bilinear(img -> h x w) - mean) / std) to multiples of patch_size; no resize when h x w is the
    image's own size (method.py:277-285, :302-305).  Forward only."""
    _need("prepare_backbone_input", img, mean, std)
    if img.dim() != 4 or img.shape[0] != 1 or mean.numel() != img.shape[1] or std.numel() != img.shape[1]:
        raise RuntimeError("wg_fused_uncertainty.prepare_backbone_input: a [1, C, H, W] image and C means / deviations are expected")
    _, Cn, H, W = img.shape
    (pt, pb), (pl, pr) = pads(h, patch_size), pads(w, patch_size)
    out = torch.empty((1, Cn, h + pt + pb, w + pl + pr), device=img.device, dtype=torch.float32)
    with torch.cuda.device(img.device):
        _native._check(_lib.wg_uncertainty_prepare(Cn, H, W, int(h), int(w), pt, pl, out.shape[2], out.shape[3], _f32(img).data_ptr(),
                                                   _f32(mean).data_ptr(), _f32(std).data_ptr(), out.data_ptr(), _stream(img.device)),
                       "wg_uncertainty_prepare")
    return out


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gamma, beta, w, b, x, kdrop, running_mean, running_var, eps, momentum, training):
        _need("uncertainty_head", gamma, beta, w, b, x, kdrop, running_mean, running_var)
        if x.dim() != 3:
            raise RuntimeError("wg_fused_uncertainty.uncertainty_head: a [C, hp, wp] feature map is expected")
        Cn, hp, wp = x.shape
        N = hp * wp
        if not (gamma.numel() == beta.numel() == w.numel() == kdrop.numel() == running_mean.numel() == running_var.numel() == Cn and b.numel() == 1):
            raise RuntimeError("wg_fused_uncertainty.uncertainty_head: C values per channel vector and one bias are expected")
        if not (running_mean.is_contiguous() and running_var.is_contiguous()):
            raise RuntimeError("wg_fused_uncertainty.uncertainty_head: the running statistics are updated in place and must be contiguous")
        dev = x.device
        x, g, be, wt, bi, k = _f32(x), _f32(gamma), _f32(beta), _f32(w), _f32(b), _f32(kdrop)
        coef = torch.empty((2, Cn), device=dev, dtype=torch.float32)
        stats = torch.empty((2, Cn), device=dev, dtype=torch.float32)
        s = torch.empty((hp, wp), device=dev, dtype=torch.float32)
        dsdl = torch.empty((hp, wp), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_uncertainty_head_stats(Cn, N, int(bool(training)), x.data_ptr(), k.data_ptr(), g.data_ptr(), be.data_ptr(),
                                                          wt.data_ptr(), float(eps), float(momentum), running_mean.data_ptr(),
                                                          running_var.data_ptr(), coef.data_ptr(), stats.data_ptr(), _stream(dev)),
                           "wg_uncertainty_head_stats")
            _native._check(_lib.wg_uncertainty_head_forward(Cn, N, x.data_ptr(), coef.data_ptr(), bi.data_ptr(), s.data_ptr(), dsdl.data_ptr(),
                                                            _stream(dev)), "wg_uncertainty_head_forward")
        ctx.save_for_backward(x, dsdl, k, stats, g, be, wt)
        ctx.shapes = (gamma.shape, beta.shape, w.shape, b.shape)
        return s

    @staticmethod
    def backward(ctx, ds):
        x, dsdl, k, stats, g, be, wt = ctx.saved_tensors
        Cn, hp, wp = x.shape
        dev = x.device
        ds = ds.contiguous().float()
        dg, dbe, dw = (torch.empty((Cn,), device=dev, dtype=torch.float32) for _ in range(3))
        db = torch.empty((1,), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_uncertainty_head_backward(Cn, hp * wp, x.data_ptr(), ds.data_ptr(), dsdl.data_ptr(), k.data_ptr(),
                                                             stats.data_ptr(), g.data_ptr(), be.data_ptr(), wt.data_ptr(), dg.data_ptr(),
                                                             dbe.data_ptr(), dw.data_ptr(), db.data_ptr(), _stream(dev)),
                           "wg_uncertainty_head_backward")
        sg, sbe, sw, sb = ctx.shapes
        return dg.view(sg), dbe.view(sbe), dw.view(sw), db.view(sb), None, None, None, None, None, None, None


def uncertainty_head(x, bn_weight, bn_bias, conv_weight, conv_bias, running_mean, running_var, kdrop, eps: float = 1e-5,
                     momentum: float = 0.1, training: bool = True) -> torch.Tensor:
    """softplus(conv_seg(bn(dropout2d(x))) + log(e - 1)) for a feature map x [C, hp, wp] -> s [hp, wp] (method.py:309-317), differentiable with
    respect to bn_weight, bn_bias, conv_weight and conv_bias ONLY (x is a constant).  kdrop [C] holds the dropout2d channel factors.  In
    training the batch statistics are used and running_mean / running_var are updated in place, as F.batch_norm does; in eval the running
    statistics are used and stay unchanged."""
    return _Head.apply(bn_weight, bn_bias, conv_weight, conv_bias, x, kdrop, running_mean, running_var, eps, momentum, training)


def uncertainty_maps(s, gt, prediction, ssim_map, msssim_map, geom: Geometry, clip_min: float):
    """-> (loss_mult [1, 1, H, W], partials): min(1 / (2 u^2), 3) with u = max(bilinear(s), clip_min) cropped to H x W, and the per-workgroup
    partial sums wg_uncertainty_finish reads.  Forward only; nothing else of full resolution is written."""
    _need("uncertainty_maps", s, gt, prediction, ssim_map, msssim_map)
    g = geom
    if tuple(s.shape) != (g.hp, g.wp) or gt.shape != prediction.shape or tuple(gt.shape[-2:]) != (g.H, g.W) or ssim_map.numel() != g.H * g.W \
            or msssim_map.numel() != g.H * g.W:
        raise RuntimeError("wg_fused_uncertainty.uncertainty_maps: shapes do not match the geometry")
    dev = s.device
    Cn = gt.numel() // (g.H * g.W)
    loss_mult = torch.empty((1, 1, g.H, g.W), device=dev, dtype=torch.float32)
    partials = torch.empty((_lib.wg_uncertainty_maps_scratch_floats(g.H, g.W),), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _native._check(_lib.wg_uncertainty_maps_forward(Cn, g.H, g.W, g.P, g.hp, g.wp, g.pad_top, g.pad_left, float(clip_min), _f32(s).data_ptr(),
                                                        _f32(gt).data_ptr(), _f32(prediction).data_ptr(), _f32(ssim_map).data_ptr(),
                                                        _f32(msssim_map).data_ptr(), loss_mult.data_ptr(), partials.data_ptr(), _stream(dev)),
                       "wg_uncertainty_maps_forward")
    return loss_mult, partials


def cosine_similarity(a: torch.Tensor, b: torch.Tensor, eps: float = COSINE_EPS) -> torch.Tensor:
    """F.cosine_similarity(a, b, dim=0) for two feature maps [C, h, w] -> [h, w]."""
    _need("cosine_similarity", a, b)
    if a.shape != b.shape or a.dim() != 3:
        raise RuntimeError("wg_fused_uncertainty.cosine_similarity: two [C, h, w] feature maps of one shape are expected")
    out = torch.empty(a.shape[1:], device=a.device, dtype=torch.float32)
    with torch.cuda.device(a.device):
        _native._check(_lib.wg_uncertainty_cosine(a.shape[0], out.numel(), float(eps), _f32(a).data_ptr(), _f32(b).data_ptr(), out.data_ptr(),
                                                  _stream(a.device)), "wg_uncertainty_cosine")
    return out


def dino_part_loss(s, feat_gt_down, feat_pred_down, geom: Geometry, clip_min: float):
    """-> (dino_part [nh, nw], partials): clip(1 - (cos^ - 0.5) / 0.5, 0, 1) from the two downsampled images' features [C, hd, wd], and the
    per-workgroup partial sums of dino_part * dino_downsample(1 / (2 u^2)), whose taps are recomputed from s.  Forward only."""
    g = geom
    _need("dino_part_loss", s, feat_gt_down, feat_pred_down)
    if tuple(s.shape) != (g.hp, g.wp) or tuple(feat_gt_down.shape[1:]) != (g.hd, g.wd):
        raise RuntimeError("wg_fused_uncertainty.dino_part_loss: shapes do not match the geometry")
    cos = cosine_similarity(feat_gt_down, feat_pred_down)
    dev = s.device
    dino_part = torch.empty((g.nh, g.nw), device=dev, dtype=torch.float32)
    partials = torch.empty((_lib.wg_uncertainty_dino_scratch_floats(g.nh, g.nw),), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _native._check(_lib.wg_uncertainty_dino_loss(g.H, g.W, g.P, g.hp, g.wp, g.pad_top, g.pad_left, float(clip_min), _f32(s).data_ptr(), g.nh,
                                                     g.nw, g.hd, g.wd, g.dpad_top, g.dpad_left, cos.data_ptr(), dino_part.data_ptr(),
                                                     partials.data_ptr(), _stream(dev)), "wg_uncertainty_dino_loss")
    return dino_part, partials


class _Loss(torch.autograd.Function):
    """s -> (loss, result [8], loss_mult); the backward pass is the gather per cell of s."""

    @staticmethod
    def forward(ctx, s, gt, prediction, ssim_map, msssim_map, feat_gt_down, feat_pred_down, geom, clip_min, reg_weight):
        g = geom
        sd = _f32(s)
        loss_mult, maps_partials = uncertainty_maps(sd, gt, prediction, ssim_map, msssim_map, g, clip_min)
        dino_part, dino_partials = dino_part_loss(sd, feat_gt_down, feat_pred_down, g, clip_min)
        dev = s.device
        result = torch.empty((8,), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_uncertainty_finish(g.H, g.W, g.nh, g.nw, float(reg_weight), maps_partials.data_ptr(), dino_partials.data_ptr(),
                                                      result.data_ptr(), _stream(dev)), "wg_uncertainty_finish")
        ctx.save_for_backward(sd, dino_part)
        ctx.args = (g, float(clip_min), float(reg_weight))
        ctx.mark_non_differentiable(result, loss_mult)
        return result[0].clone(), result, loss_mult

    @staticmethod
    def backward(ctx, grad_loss, _grad_result, _grad_mult):
        sd, dino_part = ctx.saved_tensors
        g, clip_min, reg_weight = ctx.args
        dev = sd.device
        gl = grad_loss.contiguous().reshape(1).float()
        ds = torch.empty_like(sd)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_uncertainty_maps_backward(g.H, g.W, g.P, g.hp, g.wp, g.pad_top, g.pad_left, clip_min, reg_weight, sd.data_ptr(),
                                                             g.nh, g.nw, dino_part.data_ptr(), gl.data_ptr(), ds.data_ptr(), _stream(dev)),
                           "wg_uncertainty_maps_backward")
        return (ds,) + (None,) * 9


def uncertainty_loss(s, gt, prediction, ssim_map, msssim_map, feat_gt_down, feat_pred_down, geom: Geometry, clip_min: float, reg_weight: float):
    """-> (loss, result, loss_mult): loss = mean(dino_part * down(1 / (2 u^2))) + reg_weight * mean(log u), differentiable with respect to s;
    result [8] holds RESULT_NAMES and uncertainty_loss.mean(); loss_mult [1, 1, H, W]."""
    return _Loss.apply(s, gt, prediction, ssim_map, msssim_map, feat_gt_down, feat_pred_down, geom, clip_min, reg_weight)


# ---------------------------------------------------------------------------------------------- the whole covered case
def draw_dropout_factors(channels: int, p: float, training: bool, device) -> torch.Tensor:
    """The dropout2d channel factors [C]: 0 or 1 / (1 - p) in training, 1 in eval."""
    return F.dropout2d(torch.ones((1, channels, 1, 1), device=device, dtype=torch.float32), p=p, training=training).reshape(channels)


def covered(model, gt, prediction) -> bool:
    cfg = getattr(model, "config", None)
    if cfg is None or getattr(cfg, "uncertainty_mode", None) != "dino" or getattr(cfg, "uncertainty_dino_max_size", None) is not None:
        return False
    for t in (gt, prediction):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
            return False
    if gt.shape != prediction.shape or gt.shape[0] != 1 or gt.shape[1] != 3 or gt.device != prediction.device or prediction.requires_grad:
        return False
    bn, conv = getattr(model, "bn", None), getattr(model, "conv_seg", None)
    if bn is None or conv is None:
        return False
    if any(getattr(bn, n, None) is None for n in ("weight", "bias", "running_mean", "running_var")) or isinstance(bn.momentum, bool) \
            or not isinstance(bn.momentum, (int, float)):
        return False
    w, b = getattr(conv, "weight", None), getattr(conv, "bias", None)
    if w is None or b is None or w.dim() != 4 or w.shape[0] != 1 or tuple(w.shape[2:]) != (1, 1) or w.shape[1] != bn.weight.numel():
        return False
    if tuple(getattr(conv, "stride", (1, 1))) != (1, 1) or tuple(getattr(conv, "padding", (0, 0))) != (0, 0) or getattr(conv, "groups", 1) != 1:
        return False
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, w, b, model.img_norm_mean, model.img_norm_std):
        if not (t.is_cuda and t.dtype == torch.float32 and t.device == gt.device):
            return False
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return False
    geom = Geometry(gt.shape[2], gt.shape[3], model.patch_size)
    if bn.training and geom.hp * geom.wp < 2:   # F.batch_norm refuses one value per channel
        return False
    return True


def _features(model, img, h, w, cache_entry, channels):
    """The model's own cached backbone call on prep(img, h, w) -> [C, hP / P, wP / P]; the prep launch is skipped on a cache hit."""
    P = int(model.patch_size)
    (pt, pb), (pl, pr) = pads(h, P), pads(w, P)
    shape = torch.Size((1, img.shape[1], h + pt + pb, w + pl + pr))
    if cache_entry is not None and (cache_entry, shape) in getattr(model, "_images_cache", {}):
        x = torch.empty(shape, device=img.device, dtype=torch.float32)   # the cached branch reads its shape and device only
    else:
        x = prepare_backbone_input(img, model.img_norm_mean, model.img_norm_std, h, w, P)
    with torch.no_grad():
        feat = model._get_dino_cached(x, cache_entry)
    feat = feat.detach().to(dtype=torch.float32).contiguous()
    if feat.dim() != 4 or feat.shape[0] != 1 or feat.shape[1] != channels or tuple(feat.shape[2:]) != (shape[2] // P, shape[3] // P):
        raise RuntimeError(f"wg_fused_uncertainty: the backbone returned {tuple(feat.shape)} for an input of {tuple(shape)}")
    return feat[0]


def compute_losses(model, gt, prediction, prefix="", _cache_entry=None, original=None):
    """UncertaintyModel._compute_losses(gt, prediction, prefix, _cache_entry) -> (loss, metrics, loss_mult.detach()).  `model` is duck-typed:
    config, bn, conv_seg, img_norm_mean, img_norm_std, patch_size, training, _get_dino_cached.  An uncovered call goes to
    original(model, gt, prediction, prefix, _cache_entry=_cache_entry).
    Assumption about the model's cache: a hit is predicted with the reference's own test, `(cache_entry, x.shape) in model._images_cache`
    (method.py:258), and the prepare launch is then skipped, `_get_dino_cached` being handed an UNINITIALISED tensor of the right shape and
    device.  A model whose `_get_dino_cached` decides a hit any other way (by content, by device) must not expose such keys in
    `_images_cache`; without that attribute every input is prepared."""
    if not covered(model, gt, prediction):
        if original is None:
            raise RuntimeError("wg_fused_uncertainty.compute_losses: this call is not covered (see the module docstring) and no `original` "
                               "method was given")
        return original(model, gt, prediction, prefix, _cache_entry=_cache_entry)
    import wg_fused_ssim
    cfg, bn, conv = model.config, model.bn, model.conv_seg
    gt_d, pred_d = gt.detach().contiguous(), prediction.detach().contiguous()
    _, _, H, W = gt_d.shape
    geom = Geometry(H, W, model.patch_size)
    Cn = bn.weight.numel()
    feat = _features(model, gt_d, H, W, _cache_entry, Cn)
    kdrop = draw_dropout_factors(Cn, float(cfg.uncertainty_dropout), bool(model.training), gt_d.device)
    s = uncertainty_head(feat, bn.weight, bn.bias, conv.weight, conv.bias, bn.running_mean, bn.running_var, kdrop, bn.eps, bn.momentum,
                         bn.training)
    if bn.training and getattr(bn, "num_batches_tracked", None) is not None:
        bn.num_batches_tracked.add_(1)
    ssim_map = wg_fused_ssim.ssim_down(gt_d, pred_d, max_size=400)
    msssim_map = wg_fused_ssim.msssim(gt_d, pred_d, max_size=400, min_size=80)
    feat_gt_down = _features(model, gt_d, geom.nh, geom.nw, _cache_entry, Cn)
    feat_pred_down = _features(model, pred_d, geom.nh, geom.nw, None, Cn)
    loss, result, loss_mult = uncertainty_loss(s, gt_d, pred_d, ssim_map, msssim_map, feat_gt_down, feat_pred_down, geom,
                                               float(cfg.uncertainty_clip_min), float(cfg.uncertainty_regularizer_weight))
    values = result.cpu().tolist()   # the call's one device-to-host copy
    metrics = {f"{prefix}{name}": values[i] for i, name in enumerate(RESULT_NAMES)}
    return loss, metrics, loss_mult.detach()
