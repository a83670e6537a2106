"""Fused evaluation metrics -- PSNR, SSIM, MAE and MSE of a render against its ground truth, computed on the device
(include/wg_metrics.h, csrc/metrics/metrics.hip).

    from wg_fused_metrics import frame_metrics, quantize_frame, compute_metrics
    m = frame_metrics(render, gt_uint8)                       # render: the rasterizer's float32 [3, H, W]; -> {"psnr", "ssim", "mae", "mse"}
    m = frame_metrics(render, gt_uint8, roi=(0, H, W // 2, W))   # the NeRF-W protocol's right half
    png = quantize_frame(render).cpu().numpy()                # the uint8 [H, W, 3] image the reference would have saved

The reference evaluates a test image on the host (wildgaussians/evaluation.py:331-352): the float frame is copied to the host, quantised to
8 bits by truncation (utils.py:116), turned back into float32 and run through NumPy restatements of MSE, MAE and dm_pix's SSIM, whose float64
taps make every filtered plane float64.  `frame_metrics` does the same arithmetic in one kernel and a finishing launch -- float32 values,
float32 products and differences, float64 filtering and sums -- and reads three doubles back with ONE device-to-host copy.  A raw render is
quantised while it is loaded, with the bits `quantize_frame` writes, so no intermediate tensor exists.

`compute_metrics` has the reference's signature over [..., H, W, C] NumPy arrays.  LPIPS is not restated here: the two entries come from
the callables handed in, and "lpips" is absent when none is given.

There is no CPU path: without a HIP device every function raises.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings

import numpy as np
import torch

from diff_gaussian_rasterization import _C as _native

KIND_U8, KIND_F32, KIND_F32_RENDER = 0, 1, 2
WINDOW = 11
MAX_CHANNELS = 4
MAX_SIDE = 32768


class _Desc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("kind", C.c_int32), ("reserved", C.c_int32), ("row_stride", C.c_int64), ("pixel_stride", C.c_int64),
                ("channel_stride", C.c_int64)]


_lib = _native._lib
_lib.wg_frame_quantize.restype = C.c_int
_lib.wg_frame_quantize.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.wg_image_metrics_scratch_bytes.restype = C.c_size_t
_lib.wg_image_metrics_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
_lib.wg_image_metrics.restype = C.c_int
_lib.wg_image_metrics.argtypes = [C.POINTER(_Desc), C.POINTER(_Desc)] + [C.c_int] * 7 + [C.POINTER(C.c_double), C.c_double, C.c_double,
                                                                                          C.c_void_p, C.c_void_p, C.c_void_p]


def ssim_constants(kernel_size: int = WINDOW, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, max_val: float = 1.0):
    """(taps, c1, c2) in doubles, by dm_pix's formulas as the reference evaluates them (evaluation.py:118-122, :172-173)."""
    hw = kernel_size // 2
    shift = (2 * hw - kernel_size + 1) / 2
    f_i = ((np.arange(kernel_size) - hw + shift) / sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return [float(v) for v in filt], (k1 * max_val) ** 2, (k2 * max_val) ** 2


_TAPS, _C1, _C2 = ssim_constants()
_TAPS_C = (C.c_double * WINDOW)(*_TAPS)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need_device():
    if not torch.cuda.is_available():
        raise RuntimeError("wg_fused_metrics: a HIP device is required (there is no CPU path)")


def quantize_frame(image: torch.Tensor) -> torch.Tensor:
    """float32 [C, H, W] device tensor (C = 1..4) -> uint8 [H, W, C] device tensor with the bits of the reference's
    torch.clamp(x, 0, 1).nan_to_num_(0) -> np.clip(x * 255.0, 0, 255).astype(np.uint8)."""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.dim() == 3
            and 1 <= image.shape[0] <= MAX_CHANNELS and image.numel() > 0):
        raise ValueError("wg_fused_metrics.quantize_frame: a non-empty float32 [C, H, W] tensor with 1..4 channels on a HIP device is expected")
    image = image.detach().contiguous()
    ch, H, W = image.shape
    dev = image.device
    with torch.cuda.device(dev):
        out = torch.empty((H, W, ch), device=dev, dtype=torch.uint8)
        _native._check(_lib.wg_frame_quantize(ch, H * W, image.data_ptr(), out.data_ptr(), _stream(dev)), "wg_frame_quantize")
    return out


def _on_device(x, dev, what):
    """-> a uint8 / float32 tensor on `dev` (NumPy arrays are uploaded as they lie when they can be, as a dense copy otherwise)."""
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.uint8, np.float32):
            raise ValueError(f"wg_fused_metrics: {what} must be uint8 or float32, got {x.dtype}")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)   # a read-only array: it is only read from
            x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"wg_fused_metrics: {what} must be a uint8 or float32 array or tensor")
    return x.detach().to(dev)


def _describe(t, kind, strides):
    return _Desc(t.data_ptr(), kind, 0, *strides)


def frame_metrics(pred, gt, roi=None) -> dict:
    """{"psnr", "ssim", "mae", "mse"} of one image pair as Python floats, read with one device-to-host copy.

    pred: a float32 [C, H, W] DEVICE tensor (a raw render: quantised to 8 bits on load, as the reference does before it compares), or a
          uint8 / float32 [H, W, C'] array or tensor with C' >= C, of which the first C channels are read.
    gt:   a uint8 / float32 [H, W, C] array or tensor, C = 1..4.
    roi:  (y0, y1, x0, x1): both images cropped to [y0:y1, x0:x1] first.  Each side of the crop must be at least 11.
    uint8 values are byte / 255 in float32, float32 values are clipped to [0, 1].  psnr = -10 log10(mse), inf at mse == 0."""
    _need_device()
    if getattr(gt, "ndim", None) != 3:
        raise ValueError("wg_fused_metrics.frame_metrics: gt must be [H, W, C]")
    H, W, ch = (int(s) for s in gt.shape)
    if not (1 <= ch <= MAX_CHANNELS and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"wg_fused_metrics.frame_metrics: gt of shape {tuple(gt.shape)}: 1..4 channels and sides up to {MAX_SIDE} are expected")
    if getattr(pred, "ndim", None) != 3:
        raise ValueError("wg_fused_metrics.frame_metrics: pred must have three dimensions")
    render = torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.float32 and tuple(pred.shape) == (ch, H, W)
    if not render and not (tuple(pred.shape[:2]) == (H, W) and pred.shape[2] >= ch):
        raise ValueError(f"wg_fused_metrics.frame_metrics: pred of shape {tuple(pred.shape)} fits neither [C, H, W] (a float32 device tensor) "
                         f"nor [H, W, C' >= C] for gt of shape {(H, W, ch)}")
    y0, y1, x0, x1 = (0, H, 0, W) if roi is None else (int(v) for v in roi)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W and y1 - y0 >= WINDOW and x1 - x0 >= WINDOW):
        raise ValueError(f"wg_fused_metrics.frame_metrics: roi {(y0, y1, x0, x1)} must lie inside {H} x {W} and be at least {WINDOW} x {WINDOW}")
    if torch.is_tensor(pred) and pred.is_cuda:
        dev = pred.device
    elif torch.is_tensor(gt) and gt.is_cuda:
        dev = gt.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    p, g = _on_device(pred, dev, "pred"), _on_device(gt, dev, "gt")
    if render:
        a = _describe(p, KIND_F32_RENDER, (p.stride(1), p.stride(2), p.stride(0)))
    else:
        a = _describe(p, KIND_U8 if p.dtype == torch.uint8 else KIND_F32, p.stride())
    b = _describe(g, KIND_U8 if g.dtype == torch.uint8 else KIND_F32, g.stride())
    if min(a.row_stride, a.pixel_stride, a.channel_stride, b.row_stride, b.pixel_stride, b.channel_stride) < 0:
        raise ValueError("wg_fused_metrics.frame_metrics: negative strides are not supported")
    with torch.cuda.device(dev):
        words = _lib.wg_image_metrics_scratch_bytes(ch, y1 - y0, x1 - x0) // 8
        buf = torch.empty(3 + words, device=dev, dtype=torch.float64)   # the three results, then the per-workgroup partials
        _native._check(_lib.wg_image_metrics(C.byref(a), C.byref(b), H, W, ch, y0, y1, x0, x1, _TAPS_C, _C1, _C2,
                                             buf.data_ptr() + 24, buf.data_ptr(), _stream(dev)), "wg_image_metrics")
        mse, mae, ssim = buf[:3].cpu().tolist()
    psnr = math.inf if mse == 0.0 else -10.0 * math.log10(mse)
    return {"psnr": psnr, "ssim": ssim, "mae": mae, "mse": mse}


def _as_float32(image):
    """The reference's convert_image_dtype(image, np.float32) for the dtypes handled here: what its LPIPS callables are handed."""
    return image if image.dtype == np.float32 else image.astype(np.float32) / 255.0


def compute_metrics(pred, gt, *, reduce: bool = True, run_lpips_vgg: bool = False, lpips=None, lpips_vgg=None) -> dict:
    """The reference's compute_metrics (evaluation.py:331-352) over [..., H, W, C] NumPy arrays of dtype uint8 or float32, with one
    `frame_metrics` call per image of the batch.  reduce=True: Python floats, the mean over the batch; False: float64 arrays of the batch
    shape.  "lpips" = lpips(gt, pred) and, with run_lpips_vgg, "lpips_vgg" = lpips_vgg(gt, pred) on float32 images, reduced the same way;
    "lpips" is absent when no callable is given, and run_lpips_vgg without one is an error."""
    if not (isinstance(pred, np.ndarray) and isinstance(gt, np.ndarray) and pred.ndim >= 3 and gt.ndim == pred.ndim):
        raise ValueError("wg_fused_metrics.compute_metrics: two NumPy arrays [..., H, W, C] with the same number of dimensions are expected")
    if run_lpips_vgg and lpips_vgg is None:
        raise ValueError("wg_fused_metrics.compute_metrics: run_lpips_vgg needs the lpips_vgg callable")
    full, pred = pred, pred[..., : gt.shape[-1]]
    if pred.shape != gt.shape:
        raise ValueError(f"wg_fused_metrics.compute_metrics: shapes {pred.shape} and {gt.shape} do not fit")
    batch = gt.shape[:-3]
    p3, g3 = full.reshape((-1,) + full.shape[-3:]), gt.reshape((-1,) + gt.shape[-3:])   # surplus channels are skipped through the strides
    rows = [frame_metrics(p3[i], g3[i]) for i in range(g3.shape[0])]

    def reduction(x):
        return x.mean().item() if reduce else x

    out = {k: reduction(np.array([r[k] for r in rows], dtype=np.float64).reshape(batch)) for k in ("psnr", "ssim", "mae", "mse")}
    if lpips is not None or run_lpips_vgg:
        gt32, pred32 = _as_float32(gt), _as_float32(pred)
        if lpips is not None:
            out["lpips"] = reduction(np.asarray(lpips(gt32, pred32)))
        if run_lpips_vgg:
            out["lpips_vgg"] = reduction(np.asarray(lpips_vgg(gt32, pred32)))
    return out
