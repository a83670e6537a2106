"""Fused SSIM -- opt-in replacement of the reference's `ssim()` (wildgaussians/method.py:644-673).

    from wg_fused_ssim import ssim          # same signature and results as method.py's ssim
    value = ssim(image, gt_image)                        # scalar (size_average=True)
    smap = ssim(image, gt_image, size_average=False)     # [H, W]: mean over channels, as method.py:1949 uses it

One HIP kernel computes the five 11x11 Gaussian-window statistics, the SSIM map and the three partial-derivative maps the
backward needs; one more kernel is the whole backward (include/wg_ssim.h, csrc/ssim.hip).  Gradients flow to `img1` only:
`img2` is the ground truth in the reference's use.  There is no CPU fallback: tensors must be float32 on a HIP device.

    from wg_fused_ssim import msssim, ssim_down    # the uncertainty model's two metrics (method.py:126-187), forward only
    m = msssim(gt, prediction, max_size=400, min_size=80)    # [B, H, W] in levels + 3 launches (include/wg_msssim.h, csrc/ssim.hip)
    s = ssim_down(gt, prediction, max_size=400)              # [B, H, W] in 3 launches

    from wg_fused_ssim import step_loss, step_metrics    # the train step's loss with mask, multiplier schedule and all logged metrics
    loss, stats = step_loss(image_toned, image, gt, 0.2, mask=mask, loss_mult=raw_mult, mult_threshold=1, mult_blend=p)   # method.py:1920-1965
    loss.backward(); metrics.update(step_metrics(stats))     # method.py:1968-1992 in one host copy (include/wg_step_loss.h, csrc/loss/step_loss.hip)
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_vp, _i = C.c_void_p, C.c_int
_lib.wg_ssim_forward.restype = _i
_lib.wg_ssim_forward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.wg_ssim_backward.restype = _i
_lib.wg_ssim_backward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_f = C.c_float
_lib.wg_l1_ssim_loss_scratch_floats.restype = C.c_size_t
_lib.wg_l1_ssim_loss_scratch_floats.argtypes = [_i, _i, _i]
_lib.wg_l1_ssim_loss_forward.restype = _i
_lib.wg_l1_ssim_loss_forward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.wg_l1_ssim_loss_backward.restype = _i
_lib.wg_l1_ssim_loss_backward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.wg_msssim_levels.restype = _i
_lib.wg_msssim_levels.argtypes = [_i, _i, _i]
_lib.wg_msssim_scratch_floats.restype = C.c_size_t
_lib.wg_msssim_scratch_floats.argtypes = [_i] * 7
_lib.wg_msssim_forward.restype = _i
_lib.wg_msssim_forward.argtypes = [_i] * 9 + [_vp] * 5
_lib.wg_ssim_down_scratch_floats.restype = C.c_size_t
_lib.wg_ssim_down_scratch_floats.argtypes = [_i] * 4
_lib.wg_ssim_down_forward.restype = _i
_lib.wg_ssim_down_forward.argtypes = [_i] * 7 + [_vp] * 5
_d = C.c_double
_lib.wg_step_loss_scratch_floats.restype = C.c_size_t
_lib.wg_step_loss_scratch_floats.argtypes = [_i, _i, _i]
_lib.wg_step_loss_forward.restype = _i
_lib.wg_step_loss_forward.argtypes = [_i, _i, _i] + [_vp] * 5 + [_i, _f, _f, _d] + [_vp] * 7
_lib.wg_step_loss_backward.restype = _i
_lib.wg_step_loss_backward.argtypes = [_i, _i, _i] + [_vp] * 5 + [_i, _f, _f, _d] + [_vp] * 7


def _check(img):
    if not (img.is_cuda and img.dtype == torch.float32):
        raise RuntimeError("wg_fused_ssim: float32 tensors on a HIP device are required (there is no CPU path)")


class _SSIMMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        _check(img1)
        _check(img2)
        if img1.shape != img2.shape or img1.dim() != 3:
            raise RuntimeError("wg_fused_ssim: two [C, H, W] images of the same shape are expected")
        a, b = img1.contiguous(), img2.contiguous()
        Cn, H, W = a.shape
        out = torch.empty_like(a)
        # Gradients flow to img1 only (img2 is the ground truth in the reference's use, method.py:1949); asking for img2's is an
        # error here rather than a silent None -- the reference's torch ssim() would differentiate both.
        if img2.requires_grad:
            raise RuntimeError("wg_fused_ssim: img2 is treated as a constant (the ground truth); detach it, or swap the arguments "
                               "(SSIM is symmetric) to differentiate with respect to it")
        need = ctx.needs_input_grad[0]
        ctx.have_maps = need
        d = torch.empty((3, Cn, H, W), device=a.device, dtype=torch.float32) if need else None
        stream = torch.cuda.current_stream(a.device).cuda_stream
        with torch.cuda.device(a.device):
            _native._check(_lib.wg_ssim_forward(Cn, H, W, a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                d[0].data_ptr() if need else None, d[1].data_ptr() if need else None,
                                                d[2].data_ptr() if need else None, stream), "wg_ssim_forward")
        if need:
            ctx.save_for_backward(a, b, d)
        return out

    @staticmethod
    def backward(ctx, grad_map):
        if not ctx.have_maps:
            return None, None
        a, b, d = ctx.saved_tensors
        Cn, H, W = a.shape
        g = grad_map.contiguous()
        out = torch.empty_like(a)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        with torch.cuda.device(a.device):
            _native._check(_lib.wg_ssim_backward(Cn, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                                 d[2].data_ptr(), out.data_ptr(), stream), "wg_ssim_backward")
        return out, None


def ssim_map(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """Per-channel SSIM map [C, H, W]."""
    return _SSIMMap.apply(img1, img2)


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """method.py:644-673.  Only the reference's window (11, sigma 1.5) is built in."""
    if window_size != 11:
        raise ValueError("wg_fused_ssim.ssim: only window_size=11 (the reference's default) is implemented")
    lead = img1.shape[:-3]
    if lead:  # batched input [..., C, H, W]: one launch per image
        maps = torch.stack([_SSIMMap.apply(x, y) for x, y in zip(img1.reshape(-1, *img1.shape[-3:]), img2.reshape(-1, *img2.shape[-3:]))])
        maps = maps.reshape(*lead, *img1.shape[-3:])
    else:
        maps = _SSIMMap.apply(img1, img2)
    return maps.mean() if size_average else maps.mean(-3)


class _L1SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_l1, img_ssim, gt, lambda_dssim, loss_mult):
        for t in (img_l1, img_ssim, gt):
            _check(t)
        if not (img_l1.shape == img_ssim.shape == gt.shape) or gt.dim() != 3:
            raise RuntimeError("wg_fused_ssim.l1_ssim_loss: three [C, H, W] images of the same shape are expected")
        if gt.requires_grad or (loss_mult is not None and loss_mult.requires_grad):
            raise RuntimeError("wg_fused_ssim.l1_ssim_loss: the ground truth and loss_mult are constants; detach them")
        same = img_l1 is img_ssim
        a = img_l1.contiguous()
        b = a if same else img_ssim.contiguous()
        g = gt.contiguous()
        Cn, H, W = g.shape
        m = None
        if loss_mult is not None:
            _check(loss_mult)
            m = loss_mult.expand(1, H, W).contiguous() if loss_mult.dim() == 3 else loss_mult.reshape(H, W).contiguous()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dev = g.device
        d = torch.empty((3, Cn, H, W), device=dev, dtype=torch.float32) if need else None
        scratch = torch.empty((_lib.wg_l1_ssim_loss_scratch_floats(Cn, H, W),), device=dev, dtype=torch.float32)
        out = torch.empty((3,), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native._check(_lib.wg_l1_ssim_loss_forward(Cn, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(),
                                                        float(lambda_dssim), scratch.data_ptr(), out.data_ptr(),
                                                        d[0].data_ptr() if need else None, d[1].data_ptr() if need else None,
                                                        d[2].data_ptr() if need else None, stream), "wg_l1_ssim_loss_forward")
        ctx.lam, ctx.same, ctx.have_maps = float(lambda_dssim), same, need
        if need:
            ctx.save_for_backward(a, b, g, d, m if m is not None else torch.empty(0, device=dev))
        loss, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        if not ctx.have_maps:
            return None, None, None, None, None
        a, b, g, d, m = ctx.saved_tensors
        Cn, H, W = g.shape
        gl = grad_loss.contiguous().reshape(1).float()
        ga = torch.empty_like(a)
        gb = ga if ctx.same else torch.empty_like(b)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        with torch.cuda.device(g.device):
            _native._check(_lib.wg_l1_ssim_loss_backward(Cn, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), m.data_ptr() if m.numel() else None,
                                                         ctx.lam, gl.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                         ga.data_ptr(), gb.data_ptr(), stream), "wg_l1_ssim_loss_backward")
        if ctx.same:   # autograd adds the two returned gradients of the one tensor: hand the sum over once
            return ga, None, None, None, None
        return ga, gb, None, None, None


def l1_ssim_loss(img_l1: torch.Tensor, img_ssim: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, loss_mult=None,
                 return_parts: bool = False):
    """The image loss of the reference's train step (wildgaussians/method.py:1948-1965) in two kernel launches each way:

        (1 - lambda_dssim) * (|img_l1 - gt| * loss_mult).mean() + lambda_dssim * ((1 - ssim(img_ssim, gt, size_average=False)) * loss_mult).mean()

    img_l1 is the appearance-toned render, img_ssim the raw one (pass the same tensor twice when there is only one); gt and the
    optional per-pixel loss_mult ([H, W] or [1, H, W]) are constants.  return_parts=True also returns the detached
    (l1_mean, ssim_mean) the reference logs (method.py:1970-1972)."""
    loss, parts = _L1SSIMLoss.apply(img_l1, img_ssim, gt, lambda_dssim, loss_mult)
    return (loss, parts[0], parts[1]) if return_parts else loss


# The entries of step_loss's stats vector (include/wg_step_loss.h: enum wg_step_stat), in order.
STEP_STATS = ("loss", "l1_loss", "ssim", "mse", "psnr", "l1_weighted", "dssim_weighted", "mask_percentage", "ssim_masked", "mse_masked",
              "psnr_masked", "l1_loss_masked")
_STEP_LOGGED = ("l1_loss", "ssim", "mse", "loss", "psnr")                                                   # method.py:1971-1977
_STEP_LOGGED_MASKED = ("mask_percentage", "ssim_masked", "mse_masked", "psnr_masked", "l1_loss_masked")     # method.py:1986-1992


def _plane(name, t, H, W):
    """A [H, W] or [1, H, W] float32 constant as a contiguous [H*W] plane."""
    _check(t)
    if t.requires_grad:
        raise RuntimeError(f"wg_fused_ssim.step_loss: {name} is a constant; detach it")
    if tuple(t.shape) not in ((H, W), (1, H, W)):
        raise RuntimeError(f"wg_fused_ssim.step_loss: {name} must be [H, W] or [1, H, W] = [{H}, {W}], got {list(t.shape)}")
    return t.reshape(H, W).contiguous()


class _StepLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_l1, img_ssim, gt, lambda_dssim, mask, loss_mult, mult_threshold, mult_blend, grad_mode):
        for t in (img_l1, img_ssim, gt):
            _check(t)
        if not (img_l1.shape == img_ssim.shape == gt.shape) or gt.dim() != 3:
            raise RuntimeError("wg_fused_ssim.step_loss: three [C, H, W] images of the same shape are expected")
        if gt.requires_grad:
            raise RuntimeError("wg_fused_ssim.step_loss: the ground truth is a constant; detach it")
        same = img_l1 is img_ssim
        a = img_l1.contiguous()
        b = a if same else img_ssim.contiguous()
        g = gt.contiguous()
        Cn, H, W = g.shape
        k = None if mask is None else _plane("mask", mask, H, W)
        m = None if loss_mult is None else _plane("loss_mult", loss_mult, H, W)
        n = _lib.wg_step_loss_scratch_floats(Cn, H, W)
        if n == 0:
            raise RuntimeError(f"wg_fused_ssim.step_loss: unsupported sizes ({Cn} x {H} x {W})")
        # grad_mode: the caller's torch.is_grad_enabled() (inside forward it is always off, and needs_input_grad ignores it): under no_grad
        # no derivative maps are allocated or written
        need = grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        dev = g.device
        d = torch.empty((3, Cn, H, W), device=dev, dtype=torch.float32) if need else None
        scratch = torch.empty((n // 2,), device=dev, dtype=torch.float64)   # float64 partial sums: n float32 words, 8-byte aligned
        loss = torch.empty((), device=dev, dtype=torch.float32)
        stats = torch.empty((len(STEP_STATS),), device=dev, dtype=torch.float64)
        ctx.mult_args = (int(mult_threshold is not None), float(0.0 if mult_threshold is None else mult_threshold), float(mult_blend),
                         float(lambda_dssim))
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            _native._check(_lib.wg_step_loss_forward(Cn, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), ptr(k), ptr(m), *ctx.mult_args,
                                                     scratch.data_ptr(), loss.data_ptr(), stats.data_ptr(),
                                                     d[0].data_ptr() if need else None, d[1].data_ptr() if need else None,
                                                     d[2].data_ptr() if need else None, stream), "wg_step_loss_forward")
        ctx.same, ctx.have_maps, ctx.have_mask, ctx.have_mult = same, need, k is not None, m is not None
        if need:
            none = torch.empty(0, device=dev)
            ctx.save_for_backward(a, b, g, d, none if k is None else k, none if m is None else m)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        if not ctx.have_maps:
            return (None,) * 9
        a, b, g, d, k, m = ctx.saved_tensors
        Cn, H, W = g.shape
        gl = grad_loss.contiguous().reshape(1).float()
        ga = torch.empty_like(a)
        gb = ga if ctx.same else torch.empty_like(b)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        with torch.cuda.device(g.device):
            _native._check(_lib.wg_step_loss_backward(Cn, H, W, a.data_ptr(), b.data_ptr(), g.data_ptr(), k.data_ptr() if ctx.have_mask else None,
                                                      m.data_ptr() if ctx.have_mult else None, *ctx.mult_args, gl.data_ptr(), d[0].data_ptr(),
                                                      d[1].data_ptr(), d[2].data_ptr(), ga.data_ptr(), gb.data_ptr(), stream),
                           "wg_step_loss_backward")
        if ctx.same:   # autograd adds the two returned gradients of the one tensor: hand the sum over once
            return (ga,) + (None,) * 8
        return (ga, gb) + (None,) * 7


def step_loss(image_toned: torch.Tensor, image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, *, mask=None, loss_mult=None,
              mult_threshold=None, mult_blend: float = 1.0):
    """The reference's train step between the render and loss.backward(), and the logging block behind it (wildgaussians/method.py:1920-1992,
    uncertainty_scale_grad and uncertainty_center_mult off), in two launches forward and one backward, with no host synchronisation:

        image, image_toned = scale_grads(image, mask), scale_grads(image_toned, mask)       # when mask is given: gradients * mask
        m = loss_mult;  m = (m > mult_threshold).float() when mult_threshold is given;  m = 1 + mult_blend * (m - 1)
        loss = (1 - lambda_dssim) * (|image_toned - gt| * m).mean() + lambda_dssim * ((1 - ssim(image, gt, size_average=False)) * m).mean()

    image_toned is the appearance-toned render, image the raw one (pass the same tensor twice when there is only one); gt, mask and loss_mult
    ([H, W] or [1, H, W]) are constants.  The reference's schedule (method.py:1934-1940) is mult_threshold=1 with mult_blend = 0 before the
    warm-up, p during it and 1 after it; mult_threshold=None, mult_blend=1 passes a ready-made multiplier through untouched.
    Returns (loss, stats): the differentiable float32 scalar and the float64 device vector of STEP_STATS, which step_metrics reads."""
    return _StepLoss.apply(image_toned, image, gt, lambda_dssim, mask, loss_mult, mult_threshold, mult_blend, torch.is_grad_enabled())


def step_metrics(stats: torch.Tensor, prefix: str = "") -> dict:
    """The reference's logged metrics (method.py:1971-1992, without num_gaussians) as Python floats, from step_loss's stats vector in ONE
    device-to-host copy.  The five masked entries appear exactly when step_loss was given a mask."""
    v = stats.detach().cpu().tolist()
    if len(v) != len(STEP_STATS):
        raise ValueError(f"wg_fused_ssim.step_metrics: a stats vector of {len(STEP_STATS)} entries is expected")
    by_name = dict(zip(STEP_STATS, v))
    names = _STEP_LOGGED + (_STEP_LOGGED_MASKED if not math.isnan(by_name["mask_percentage"]) else ())
    return {prefix + n: by_name[n] for n in names}


def _area_size(H: int, W: int, scale_factor: float):
    """The output size of F.interpolate(scale_factor=..., mode='area'): floor(size * scale) in Python doubles."""
    return int(math.floor(float(H * scale_factor))), int(math.floor(float(W * scale_factor)))


def msssim_plan(H: int, W: int, max_size=None, min_size: int = 200) -> list:
    """The (h, w) of every pyramid level of msssim(x, y, max_size, min_size) for H x W images (method.py:171-183), level 0 first.
    Pure host arithmetic: the area resize's floor(size * scale) in Python doubles, then avg_pool2d(2) while both sides exceed min_size."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or min_size < 1:
        raise ValueError("msssim_plan: H, W and min_size must be positive")
    h, w = H, W
    if max_size is not None:
        h, w = _area_size(H, W, min(1, max(max_size / H, max_size / W)))
        if h < 1 or w < 1:
            raise ValueError(f"msssim_plan: max_size={max_size} resizes {H}x{W} to an empty image")
    levels = [(h, w)]
    while h > min_size and w > min_size:
        h, w = h // 2, w // 2
        levels.append((h, w))
    return levels


def _metric_inputs(name, x, y):
    for t in (x, y):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"wg_fused_ssim.{name}: float32 tensors on a HIP device are required (there is no CPU path)")
        if t.requires_grad:
            raise RuntimeError(f"wg_fused_ssim.{name} is forward-only (the reference calls it on detached images); detach the inputs")
    if x.shape != y.shape or x.dim() not in (3, 4):
        raise RuntimeError(f"wg_fused_ssim.{name}: two [B, C, H, W] or [C, H, W] images of the same shape are expected")
    if x.device != y.device:
        raise RuntimeError(f"wg_fused_ssim.{name}: both images must be on the same device")
    batched = x.dim() == 4
    a, b = x.contiguous(), y.contiguous()
    if not batched:
        a, b = a[None], b[None]
    return a, b, batched


def msssim(x: torch.Tensor, y: torch.Tensor, max_size=None, min_size: int = 200) -> torch.Tensor:
    """method.py:171-187, forward only: [B, C, H, W] -> [B, H, W] (also [C, H, W] -> [H, W]).  One launch per pyramid level plus the
    resize, the combine and the finish kernel (csrc/ssim.hip); bit-reproducible."""
    a, b, batched = _metric_inputs("msssim", x, y)
    B, Cn, H, W = a.shape
    h0, w0 = msssim_plan(H, W, max_size, min_size)[0]
    resize = (h0, w0) != (H, W)   # an area resize to the same size is the identity: its launch is skipped
    final_upsample = max_size is not None
    dev = a.device
    n = _lib.wg_msssim_scratch_floats(B, Cn, H, W, h0, w0, int(min_size))
    if n == 0:
        raise RuntimeError(f"wg_fused_ssim.msssim: unsupported sizes (B*C={B * Cn}, {H}x{W} -> {h0}x{w0}, min_size={min_size})")
    scratch = torch.empty((n,), device=dev, dtype=torch.float32)
    out = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native._check(_lib.wg_msssim_forward(B, Cn, H, W, h0, w0, int(resize), int(final_upsample), int(min_size), a.data_ptr(), b.data_ptr(),
                                              scratch.data_ptr(), out.data_ptr(), stream), "wg_msssim_forward")
    return out if batched else out[0]


def ssim_down(x: torch.Tensor, y: torch.Tensor, max_size=None) -> torch.Tensor:
    """method.py:126-135, forward only: [B, C, H, W] -> [B, H, W] (also [C, H, W] -> [H, W]).  Area resize (down OR up: there is no
    min(1, .) here), the product-form SSIM, the channel mean, bilinear upsampling back: three launches."""
    a, b, batched = _metric_inputs("ssim_down", x, y)
    B, Cn, H, W = a.shape
    h0, w0 = H, W
    if max_size is not None:
        h0, w0 = _area_size(H, W, max(max_size / H, max_size / W))
        if h0 < 1 or w0 < 1:
            raise RuntimeError(f"wg_fused_ssim.ssim_down: max_size={max_size} resizes {H}x{W} to an empty image")
    dev = a.device
    n = _lib.wg_ssim_down_scratch_floats(B, Cn, h0, w0)
    if n == 0:
        raise RuntimeError(f"wg_fused_ssim.ssim_down: unsupported sizes (B*C={B * Cn}, {H}x{W} -> {h0}x{w0})")
    scratch = torch.empty((n,), device=dev, dtype=torch.float32)
    out = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native._check(_lib.wg_ssim_down_forward(B, Cn, H, W, h0, w0, int(max_size is not None), a.data_ptr(), b.data_ptr(), scratch.data_ptr(),
                                                 out.data_ptr(), stream), "wg_ssim_down_forward")
    return out if batched else out[0]
