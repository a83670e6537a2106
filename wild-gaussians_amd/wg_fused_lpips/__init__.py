"""Fused LPIPS v0.1 on the AlexNet and VGG16 trunks -- opt-in replacement of what `evaluation._lpips` (wildgaussians/evaluation.py:255-291) runs
per test image: `LPIPS.forward` (wildgaussians/_metrics_lpips.py:149-180) as HIP kernels (include/wg_lpips.h, csrc/lpips/lpips.hip): forward only,
float32 throughout, implicit-GEMM convolutions on the matrix cores, both images as one batch.

    from wg_fused_lpips import LPIPS
    fused = LPIPS.from_module(lp_net)            # the caller's own LPIPS object: its weights are read, nothing is downloaded
    d = fused(pred, gt)                          # device tensors [B, 3, H, W] or [3, H, W] in [0, 1] -> [B]
    d, layers = fused(pred, gt, per_layer=True)  # layers [B, 5]
    taps = fused.features(x)                     # the five taps of the scaled images, [N, C_l, h_l, w_l]

Covered case, decided on the module alone (`structure_covered`): `pnet_type` alex or vgg / vgg16 with exactly the layers of
_metrics_lpips.py:286-364 (every Conv2d's window, stride, padding and widths, every pool's window and stride 2 without padding or ceil_mode),
`lpips=True`, `spatial=False`, version "0.1", eval mode, float32 parameters.  Nothing else is served: `from_module` raises on another module
and `__call__` on another input, there is no PyTorch path.  Inputs are float32 tensors on the HIP device of the packed weights, of any strides
(a planar render, an uploaded H x W x 3 array seen through `permute`, a crop): they are read in place, the caller's clip, `* 2 - 1` and scaling
layer are applied on load.  H, W >= 31 (alex) or 16 (vgg).

Weights are repacked on the device into [Cout][KH][KW][Cin] (rows padded to a multiple of 4 floats) at construction, and again when any
parameter's or buffer's `_version` or `data_ptr()` has changed, so a `load_state_dict`, an in-place edit or a `.to(...)` is seen.  The module
may live on the CPU: the packed copies live on the HIP device given to `from_module` (default: the module's, else the current one).
Scratch (`wg_lpips_scratch_floats`; 1.97 GB for a 1600x1200 pair on vgg, 122 MB on alex) is owned by the object: one buffer, kept between calls and
replaced by a larger one when a call needs more.  No atomics: two calls give the same bits, and image b of a batch gives the bits of the
single call.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

ALEX, VGG = 0, 1
TAPS, MAX_CONVS, HEAD_PIXELS = 5, 13, 256
MIN_SIDE = {ALEX: 31, VGG: 16}
# (Cin, Cout, window, stride, pad, pool window before it or 0, tap after its ReLU)
_V = lambda cin, cout, pool=0, tap=False: (cin, cout, 3, 1, 1, pool, tap)
CONVS = {
    ALEX: [(3, 64, 11, 4, 2, 0, True), (64, 192, 5, 1, 2, 3, True), (192, 384, 3, 1, 1, 3, True), (384, 256, 3, 1, 1, 0, True),
           (256, 256, 3, 1, 1, 0, True)],
    VGG: [_V(3, 64), _V(64, 64, tap=True), _V(64, 128, pool=2), _V(128, 128, tap=True), _V(128, 256, pool=2), _V(256, 256), _V(256, 256, tap=True),
          _V(256, 512, pool=2), _V(512, 512), _V(512, 512, tap=True), _V(512, 512, pool=2), _V(512, 512), _V(512, 512, tap=True)],
}
TAP_CHANNELS = {net: [c[1] for c in convs if c[6]] for net, convs in CONVS.items()}
NET_OF = {"alex": ALEX, "vgg": VGG, "vgg16": VGG}


class Image(C.Structure):
    _fields_ = [("data", _vp), ("batch_stride", _i64), ("row_stride", _i64), ("pixel_stride", _i64), ("channel_stride", _i64)]


class Args(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("net", _i32), ("B", _i32), ("H", _i32), ("W", _i32), ("in0", Image), ("in1", Image),
                ("shift", _vp), ("scale", _vp), ("conv_w", _vp * MAX_CONVS), ("conv_b", _vp * MAX_CONVS), ("lin_w", _vp * TAPS),
                ("scratch", _vp), ("scratch_floats", _i64), ("out", _vp), ("per_layer", _vp), ("stream", _vp)]


class ConvArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("N", _i32), ("IH", _i32), ("IW", _i32), ("Cin", _i32), ("Cout", _i32), ("K", _i32), ("stride", _i32),
                ("pad", _i32), ("x", _vp), ("in0", Image), ("in1", Image), ("N0", _i32), ("shift", _vp), ("scale", _vp), ("w", _vp), ("bias", _vp),
                ("y", _vp), ("stream", _vp)]


for _name, _res, _args in (("wg_lpips_scratch_floats", _i64, [_i32] * 4),
                           ("wg_lpips", C.c_int, [C.POINTER(Args)]),
                           ("wg_lpips_conv", C.c_int, [C.POINTER(ConvArgs)]),
                           ("wg_lpips_pool", C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
                           ("wg_lpips_head", C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp])):
    getattr(_lib, _name).restype = _res
    getattr(_lib, _name).argtypes = _args


def scratch_floats(net: int, B: int, H: int, W: int) -> int:
    n = _lib.wg_lpips_scratch_floats(int(net), int(B), int(H), int(W))
    if n < 0:
        raise RuntimeError(f"wg_lpips_scratch_floats({net}, {B}, {H}, {W}) was refused ({n})")
    return n


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _device_f32(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"wg_fused_lpips.{what}: float32 tensors on a HIP device are required (there is no CPU path)")


def _image(t) -> Image:
    """The description of a [B, 3, H, W] tensor of any strides."""
    sb, sc, sy, sx = t.stride()
    return Image(t.data_ptr(), sb, sy, sx, sc)


# ------------------------------------------------------------------------------------------------ the stages alone
def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, KH, KW] -> [Cout, Kpad]: rows (ky, kx, ci), padded with zeros to a multiple of 4 floats."""
    cout = w.shape[0]
    rows = w.detach().float().permute(0, 2, 3, 1).reshape(cout, -1)
    return F.pad(rows, (0, -rows.shape[1] % 4)).contiguous()


def _conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, K: int, stride: int, pad: int) -> torch.Tensor:
    """relu(conv2d(x) + bias) on channels-last tensors: x [N, IH, IW, Cin] contiguous -> [N, OH, OW, Cout]."""
    for t in (x, w_packed, bias):
        _device_f32(t, "conv")
    x = x.contiguous()
    N, IH, IW, Cin = (int(v) for v in x.shape)
    Cout = int(w_packed.shape[0])
    a = ConvArgs(struct_size=C.sizeof(ConvArgs), N=N, IH=IH, IW=IW, Cin=Cin, Cout=Cout, K=K, stride=stride, pad=pad)
    y = torch.empty((N, max(_conv_out(IH, K, stride, pad), 0), max(_conv_out(IW, K, stride, pad), 0), Cout), device=x.device, dtype=torch.float32)
    a.x, a.w, a.bias, a.y, a.stream = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), y.data_ptr(), _stream(x.device)
    with torch.cuda.device(x.device):
        _native._check(_lib.wg_lpips_conv(C.byref(a)), "wg_lpips_conv")
    return y


def conv_images(in0, in1, shift, scale, w_packed, bias, K, stride, pad) -> torch.Tensor:
    """The first layer: images [N0, 3, H, W] and (or None) [N1, 3, H, W] of any strides, scaled on load -> [N0 + N1, OH, OW, Cout]."""
    for t in (in0, shift, scale, w_packed, bias) + (() if in1 is None else (in1,)):
        _device_f32(t, "conv_images")
    N0, _, IH, IW = (int(v) for v in in0.shape)
    N = N0 + (0 if in1 is None else int(in1.shape[0]))
    Cout = int(w_packed.shape[0])
    a = ConvArgs(struct_size=C.sizeof(ConvArgs), N=N, IH=IH, IW=IW, Cin=3, Cout=Cout, K=K, stride=stride, pad=pad, N0=N0)
    a.in0 = _image(in0)
    a.in1 = _image(in0 if in1 is None else in1)
    y = torch.empty((N, max(_conv_out(IH, K, stride, pad), 0), max(_conv_out(IW, K, stride, pad), 0), Cout), device=in0.device, dtype=torch.float32)
    a.shift, a.scale, a.w, a.bias, a.y, a.stream = shift.data_ptr(), scale.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), y.data_ptr(), \
        _stream(in0.device)
    with torch.cuda.device(in0.device):
        _native._check(_lib.wg_lpips_conv(C.byref(a)), "wg_lpips_conv")
    return y


def pool(x: torch.Tensor, window: int) -> torch.Tensor:
    """Max pool, stride 2, floor, no padding, on a channels-last tensor [N, IH, IW, C]."""
    _device_f32(x, "pool")
    x = x.contiguous()
    N, IH, IW, Cn = (int(v) for v in x.shape)
    y = torch.empty((N, max((IH - window) // 2 + 1, 0), max((IW - window) // 2 + 1, 0), Cn), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _native._check(_lib.wg_lpips_pool(x.data_ptr(), N, IH, IW, Cn, int(window), y.data_ptr(), _stream(x.device)), "wg_lpips_pool")
    return y


def head(f: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """One tap's value: f [2 B, h, w, C] channels-last (images b and B + b are compared), lin [C] -> [B]."""
    _device_f32(f, "head")
    _device_f32(lin, "head")
    f = f.contiguous()
    N2, h, w, Cn = (int(v) for v in f.shape)
    if N2 % 2 or N2 < 2:
        raise RuntimeError("wg_fused_lpips.head: an even number of images is required")
    B = N2 // 2
    partials = torch.empty((B * ((h * w + HEAD_PIXELS - 1) // HEAD_PIXELS),), device=f.device, dtype=torch.float64)
    out = torch.empty((B,), device=f.device, dtype=torch.float32)
    with torch.cuda.device(f.device):
        _native._check(_lib.wg_lpips_head(f.data_ptr(), B, h, w, Cn, lin.contiguous().data_ptr(), partials.data_ptr(), out.data_ptr(), _stream(f.device)),
                       "wg_lpips_head")
    return out


# ------------------------------------------------------------------------------------------------ the module's structure
def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _trunk_layers(lp_net):
    """The trunk's modules in order, slice after slice."""
    for i in range(1, 6):
        for m in getattr(lp_net.net, f"slice{i}"):
            yield i - 1, m


def _walk(lp_net, net):
    """-> (the Conv2d modules in order, the `lin` Conv2d modules) when the module is exactly the covered trunk, else None."""
    want = []          # what each module has to be, in order: ("conv", spec) / ("relu",) / ("pool", window), and the slice it ends
    for cin, cout, k, s, p, pool_w, tap in CONVS[net]:
        if pool_w:
            want.append(("pool", pool_w))
        want.append(("conv", (cin, cout, k, s, p)))
        want.append(("relu", tap))
    got = list(_trunk_layers(lp_net))
    if len(got) != len(want):
        return None
    convs, tap = [], 0
    for j, ((sl, m), w) in enumerate(zip(got, want)):
        kind = type(m).__name__
        if w[0] == "conv":
            cin, cout, k, s, p = w[1]
            if kind != "Conv2d" or tuple(m.weight.shape) != (cout, cin, k, k) or m.bias is None or tuple(m.bias.shape) != (cout,):
                return None
            if _pair(m.stride) != (s, s) or _pair(m.padding) != (p, p) or _pair(m.dilation) != (1, 1) or m.groups != 1 or \
                    getattr(m, "padding_mode", "zeros") != "zeros":
                return None
            convs.append(m)
        elif w[0] == "relu":
            if kind != "ReLU":
                return None
            last_of_slice = j + 1 == len(got) or got[j + 1][0] != sl
            if w[1] != last_of_slice or (w[1] and sl != tap):   # a tap is what ends a slice, and slice l ends with tap l
                return None
            tap += bool(w[1])
        else:
            if kind != "MaxPool2d" or _pair(m.kernel_size) != (w[1], w[1]) or _pair(m.stride) != (2, 2) or _pair(m.padding) != (0, 0) or \
                    _pair(m.dilation) != (1, 1) or m.ceil_mode:
                return None
            if j + 1 == len(got) or got[j + 1][0] != sl:   # a slice does not end with a pool
                return None
    lins = []
    if len(lp_net.lins) != TAPS:
        return None
    for lin, cn in zip(lp_net.lins, TAP_CHANNELS[net]):
        mods = list(lin.model)
        if any(type(m).__name__ != "Dropout" for m in mods[:-1]):   # inactive: the module is in eval mode
            return None
        c = mods[-1]
        if type(c).__name__ != "Conv2d" or tuple(c.weight.shape) != (1, cn, 1, 1) or c.bias is not None:
            return None
        lins.append(c)
    return convs, lins


def structure_covered(lp_net) -> bool:
    """Is this module the covered model, wherever its parameters live?  Duck-typed: nothing is imported from the caller."""
    try:
        net = NET_OF.get(lp_net.pnet_type)
        if net is None or lp_net.lpips is not True or lp_net.spatial is not False or lp_net.version != "0.1" or lp_net.training:
            return False
        found = _walk(lp_net, net)
        if found is None:
            return False
        shift, scale = lp_net.scaling_layer.shift, lp_net.scaling_layer.scale
        if shift.numel() != 3 or scale.numel() != 3:
            return False
        tensors = [shift, scale] + [t for m in found[0] for t in (m.weight, m.bias)] + [m.weight for m in found[1]]
        return all(t.dtype == torch.float32 for t in tensors)
    except (AttributeError, TypeError, ValueError):
        return False


class LPIPS:
    """The fused metric of one LPIPS module.  Build it with `LPIPS.from_module`."""

    def __init__(self, lp_net, device=None):
        if not structure_covered(lp_net):
            raise RuntimeError("wg_fused_lpips.LPIPS: this module is not the covered model (see the module docstring)")
        self.module = lp_net
        self.net = NET_OF[lp_net.pnet_type]
        if device is None:
            p = lp_net.scaling_layer.shift
            device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("wg_fused_lpips.LPIPS: a HIP device is required (there is no CPU path)")
        self._scratch = None
        self._pack()

    @classmethod
    def from_module(cls, lp_net, device=None):
        return cls(lp_net, device)

    # ------------------------------------------------------------------------------------------ weights
    def _current_stamp(self):
        return tuple((t.data_ptr(), t._version) for t in self._params)

    def _pack(self):
        convs, lins = _walk(self.module, self.net)
        sl = self.module.scaling_layer
        self._params = [sl.shift, sl.scale] + [t for m in convs for t in (m.weight, m.bias)] + [m.weight for m in lins]
        dev = self.device
        with torch.no_grad():
            self._shift = sl.shift.detach().to(dev).reshape(3).contiguous()
            self._scale = sl.scale.detach().to(dev).reshape(3).contiguous()
            self._conv_w = [pack_conv_weight(m.weight.to(dev)) for m in convs]
            self._conv_b = [m.bias.detach().to(dev).contiguous() for m in convs]
            self._lin_w = [m.weight.detach().to(dev).reshape(-1).contiguous() for m in lins]
        a = self._args = Args()
        a.struct_size, a.net = C.sizeof(Args), self.net
        a.shift, a.scale = self._shift.data_ptr(), self._scale.data_ptr()
        for i, (w, b) in enumerate(zip(self._conv_w, self._conv_b)):
            a.conv_w[i], a.conv_b[i] = w.data_ptr(), b.data_ptr()
        for i, w in enumerate(self._lin_w):
            a.lin_w[i] = w.data_ptr()
        self._stamp = self._current_stamp()

    def refresh(self):
        """Walk the module again: after a Parameter object was replaced."""
        if not structure_covered(self.module):
            raise RuntimeError("wg_fused_lpips.LPIPS: the module has left the covered case since construction")
        self._pack()

    def _fresh(self):
        if self._stamp != self._current_stamp() or self.module.training:
            self.refresh()

    # ------------------------------------------------------------------------------------------ the covered case
    def input_covered(self, pred, gt) -> bool:
        if not (torch.is_tensor(pred) and torch.is_tensor(gt) and pred.shape == gt.shape and pred.dim() in (3, 4)):
            return False
        if not all(t.is_cuda and t.device == self.device and t.dtype == torch.float32 for t in (pred, gt)):
            return False
        B = 1 if pred.dim() == 3 else int(pred.shape[0])
        Cn, H, W = (int(v) for v in pred.shape[-3:])
        return Cn == 3 and B >= 1 and min(H, W) >= MIN_SIDE[self.net] and _lib.wg_lpips_scratch_floats(self.net, B, H, W) > 0

    def _scratch_for(self, need):
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = None   # the old buffer goes before the new one comes
            self._scratch = torch.empty((need,), device=self.device, dtype=torch.float32)
        return self._scratch

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor, per_layer: bool = False, _guard_floats: int = 0):
        """-> [B] (and [B, 5] with `per_layer`).  `_guard_floats` (tests): outputs and scratch are allocated with that many floats on either
        side, filled with a pattern, and returned after the results as (out buffer, per-layer buffer, scratch buffer)."""
        self._fresh()
        if not self.input_covered(pred, gt):
            raise RuntimeError("wg_fused_lpips.LPIPS: this input is not covered (two float32 [B, 3, H, W] or [3, H, W] tensors of one shape on the "
                               "packed weights' HIP device, H and W at or above the trunk's minimum); there is no PyTorch path")
        pred, gt = pred.detach(), gt.detach()
        if pred.dim() == 3:
            pred, gt = pred[None], gt[None]
        B, _, H, W = (int(v) for v in pred.shape)
        dev, g = self.device, int(_guard_floats)
        need = scratch_floats(self.net, B, H, W)
        if g:
            out_buf = torch.full((B + 2 * g,), 12345.0, device=dev, dtype=torch.float32)
            layer_buf = torch.full((B * TAPS + 2 * g,), 12345.0, device=dev, dtype=torch.float32)
            scratch = torch.full((need + 2 * g,), 12345.0, device=dev, dtype=torch.float32)
        else:
            out_buf = torch.empty((B,), device=dev, dtype=torch.float32)
            layer_buf = torch.empty((B * TAPS,), device=dev, dtype=torch.float32) if per_layer else None
            scratch = self._scratch_for(need)
        out = out_buf[g:g + B]
        layers = layer_buf[g:g + B * TAPS].view(B, TAPS) if layer_buf is not None else None
        a = self._args
        a.B, a.H, a.W = B, H, W
        a.in0, a.in1 = _image(pred), _image(gt)
        a.scratch, a.scratch_floats = scratch[g:].data_ptr(), need
        a.out, a.per_layer, a.stream = out.data_ptr(), (layers.data_ptr() if layers is not None else None), _stream(dev)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_lpips(C.byref(a)), "wg_lpips")
        if g:
            return out, layers, out_buf, layer_buf, scratch
        return (out, layers) if per_layer else out

    def features(self, x: torch.Tensor):
        """[N, 3, H, W] or [3, H, W] in [0, 1] -> the five taps of the scaled images as [N, C_l, h_l, w_l] tensors (views of channels-last
        storage), through the stage entry points."""
        self._fresh()
        if not (torch.is_tensor(x) and x.is_cuda and x.device == self.device and x.dtype == torch.float32 and x.dim() in (3, 4)
                and x.shape[-3] == 3 and min(x.shape[-2:]) >= MIN_SIDE[self.net]):
            raise RuntimeError("wg_fused_lpips.LPIPS.features: this input is not covered (see __call__)")
        x = x.detach()
        if x.dim() == 3:
            x = x[None]
        taps, cur = [], None
        for (cin, cout, k, s, p, pool_w, tap), w, b in zip(CONVS[self.net], self._conv_w, self._conv_b):
            if pool_w:
                cur = pool(cur, pool_w)
            cur = conv_images(x, None, self._shift, self._scale, w, b, k, s, p) if cur is None else conv(cur, w, b, k, s, p)
            if tap:
                taps.append(cur.permute(0, 3, 1, 2))
        return taps
