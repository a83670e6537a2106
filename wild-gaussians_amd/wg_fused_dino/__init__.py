"""Fused frozen DINOv2 ViT-S/14 feature extractor -- opt-in replacement of the backbone call of `UncertaintyModel._get_dino_cached`
(wildgaussians/method.py:257-265): `backbone.get_intermediate_layers(x, n=[k], reshape=True)[-1]` (wildgaussians/dinov2.py:789-813) as HIP
kernels (include/wg_dino.h, csrc/dino/vit.hip): forward only, float32 throughout, blocks 0..k only, no N x N tensor anywhere.

    from wg_fused_dino import DinoFeatures
    if DinoFeatures.covers(backbone, x):
        feat = DinoFeatures(backbone).features(x)        # [B, 384, H / 14, W / 14]; block = backbone.num_heads - 1 unless given

Covered case: what `dinov2_vits14_reg` builds (patch 14, embed 384, 6 heads x 64, `Mlp` blocks 384 -> 1536 -> 384 with the exact GELU, every bias,
LayerScale on both branches, 1 class token and 4 register tokens), float32 parameters and a float32 [B, 3, H, W] input with H, W multiples of 14
on one HIP device, blocks not chunked, no drop path or dropout that is active, no masks.  Nothing else is served: `features` raises on an
uncovered input, there is no PyTorch path.

The position embedding for an h x w grid is prepared by torch exactly as `interpolate_pos_encoding` (dinov2.py:670-702) does -- bicubic
F.interpolate with the module's `interpolate_antialias`, `size=` or `scale_factor=` by its `interpolate_offset`, the parameter as it is when
h == w == M -- once per grid size, and cached; the kernels only add it.

Weights are packed once (contiguous float32 views of the module's own parameters where they already are that; no copy then) and repacked when any
used parameter's `_version` or `data_ptr()` has changed, so a `load_state_dict`, an in-place edit or a `.to(...)` after construction is seen.
No atomics: two calls give the same bits, and image b of a batch gives the bits of the single-image call.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_vp, _i32, _i64, _f = C.c_void_p, C.c_int32, C.c_int64, C.c_float

PATCH, EMBED, HEADS, HEAD_DIM, HIDDEN, LEAD_TOKENS, MAX_BLOCKS = 14, 384, 6, 64, 1536, 5, 12
REGISTER_TOKENS = LEAD_TOKENS - 1
BLOCK_FIELDS = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2")


class Block(C.Structure):
    _fields_ = [(n, _vp) for n in BLOCK_FIELDS]


class Args(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("B", _i32), ("H", _i32), ("W", _i32), ("num_blocks", _i32), ("eps", _f), ("gemm_tiling", _i32),
                ("image", _vp), ("patch_w", _vp), ("patch_b", _vp), ("pos", _vp), ("cls_token", _vp), ("reg_tokens", _vp),
                ("blocks", Block * MAX_BLOCKS), ("norm_w", _vp), ("norm_b", _vp), ("scratch", _vp), ("scratch_floats", _i64), ("out", _vp),
                ("stream", _vp)]


for _name, _res, _args in (("wg_dino_scratch_floats", _i64, [_i32] * 3),
                           ("wg_dino_features", C.c_int, [C.POINTER(Args)]),
                           ("wg_dino_attention", C.c_int, [_vp, _i32, _i32, _vp, _vp])):
    getattr(_lib, _name).restype = _res
    getattr(_lib, _name).argtypes = _args


def scratch_floats(B: int, h: int, w: int) -> int:
    n = _lib.wg_dino_scratch_floats(int(B), int(h), int(w))
    if n < 0:
        raise RuntimeError(f"wg_dino_scratch_floats({B}, {h}, {w}) was refused ({n})")
    return n


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _linear_ok(m, out_f, in_f):
    w, b = getattr(m, "weight", None), getattr(m, "bias", None)
    return torch.is_tensor(w) and torch.is_tensor(b) and tuple(w.shape) == (out_f, in_f) and tuple(b.shape) == (out_f,)


def _norm_ok(m):
    w, b = getattr(m, "weight", None), getattr(m, "bias", None)
    return torch.is_tensor(w) and torch.is_tensor(b) and tuple(w.shape) == (EMBED,) and tuple(b.shape) == (EMBED,) and \
        isinstance(getattr(m, "eps", None), float) and m.eps > 0


def _used_parameters(backbone, nblocks):
    """Every tensor the extractor reads, in the order it is packed."""
    yield backbone.patch_embed.proj.weight
    yield backbone.patch_embed.proj.bias
    yield backbone.pos_embed
    yield backbone.cls_token
    yield backbone.register_tokens
    for blk in list(backbone.blocks)[:nblocks]:
        for t in (blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.attn.proj.bias, blk.ls1.gamma,
                  blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.ls2.gamma):
            yield t
    yield backbone.norm.weight
    yield backbone.norm.bias


def structure_covered(backbone, block=None) -> bool:
    """Is this module the covered model, wherever its parameters live (widths, biases, LayerScale, 1 + 4 leading tokens, plain blocks, no drop
    path)?  Duck-typed: nothing is imported from the caller."""
    try:
        if getattr(backbone, "chunked_blocks", False) or int(backbone.patch_size) != PATCH or int(backbone.num_heads) != HEADS:
            return False
        blocks = list(backbone.blocks)
        k = int(backbone.num_heads) - 1 if block is None else int(block)
        if not 0 <= k < min(len(blocks), MAX_BLOCKS):
            return False
        proj = backbone.patch_embed.proj
        if tuple(proj.weight.shape) != (EMBED, 3, PATCH, PATCH) or proj.bias is None or tuple(proj.bias.shape) != (EMBED,):
            return False
        if tuple(getattr(proj, "stride", (PATCH, PATCH))) != (PATCH, PATCH) or tuple(getattr(proj, "padding", (0, 0))) != (0, 0):
            return False
        if type(getattr(backbone.patch_embed, "norm", torch.nn.Identity())).__name__ != "Identity":
            return False
        if tuple(backbone.cls_token.shape) != (1, 1, EMBED) or backbone.register_tokens is None or \
                tuple(backbone.register_tokens.shape) != (1, REGISTER_TOKENS, EMBED):
            return False
        pe = backbone.pos_embed
        M = int(math.sqrt(pe.shape[1] - 1))
        if pe.dim() != 3 or pe.shape[0] != 1 or pe.shape[2] != EMBED or M * M != pe.shape[1] - 1 or M < 1:
            return False
        if not _norm_ok(backbone.norm):
            return False
        eps = backbone.norm.eps
        for blk in blocks[:k + 1]:
            if not (_norm_ok(blk.norm1) and _norm_ok(blk.norm2) and blk.norm1.eps == eps and blk.norm2.eps == eps):
                return False
            if not (_linear_ok(blk.attn.qkv, 3 * EMBED, EMBED) and _linear_ok(blk.attn.proj, EMBED, EMBED) and int(blk.attn.num_heads) == HEADS):
                return False
            if not (_linear_ok(blk.mlp.fc1, HIDDEN, EMBED) and _linear_ok(blk.mlp.fc2, EMBED, HIDDEN)):
                return False
            act = getattr(blk.mlp, "act", None)
            if type(act).__name__ != "GELU" or getattr(act, "approximate", "none") != "none":
                return False
            for ls in (blk.ls1, blk.ls2):
                g = getattr(ls, "gamma", None)
                if not torch.is_tensor(g) or tuple(g.shape) != (EMBED,):
                    return False
            for dp in (getattr(blk, "drop_path1", None), getattr(blk, "drop_path2", None)):
                if dp is not None and type(dp).__name__ != "Identity" and (float(getattr(dp, "drop_prob", 0.0) or 0.0) > 0.0 and backbone.training):
                    return False
            if backbone.training and float(getattr(blk, "sample_drop_ratio", 0.0) or 0.0) > 0.0:
                return False
            for drop in (getattr(blk.attn, "attn_drop", None), getattr(blk.attn, "proj_drop", None), getattr(blk.mlp, "drop", None)):
                if drop is not None and backbone.training and float(getattr(drop, "p", 0.0)) > 0.0:
                    return False
        return True
    except (AttributeError, TypeError, ValueError):
        return False


def model_covered(backbone, block=None) -> bool:
    """structure_covered, and every parameter that is read is float32 on one HIP device."""
    if not structure_covered(backbone, block):
        return False
    k = int(backbone.num_heads) - 1 if block is None else int(block)
    dev = backbone.pos_embed.device
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == dev for t in _used_parameters(backbone, k + 1))


def prepare_pos_embed(backbone, h: int, w: int) -> torch.Tensor:
    """-> [1 + h w, 384]: `interpolate_pos_encoding` (dinov2.py:670-702) for an h x w patch grid, class row first."""
    pe = backbone.pos_embed.detach().float()
    Npos = pe.shape[1] - 1
    if h * w == Npos and h == w:
        return pe[0].contiguous()
    M = int(math.sqrt(Npos))
    kwargs = {}
    offset = getattr(backbone, "interpolate_offset", 0.0)
    if offset:
        kwargs["scale_factor"] = (float(h + offset) / M, float(w + offset) / M)
    else:
        kwargs["size"] = (h, w)
    patch = F.interpolate(pe[:, 1:].reshape(1, M, M, EMBED).permute(0, 3, 1, 2), mode="bicubic",
                          antialias=bool(getattr(backbone, "interpolate_antialias", False)), **kwargs)
    if tuple(patch.shape[-2:]) != (h, w):
        raise RuntimeError(f"wg_fused_dino: the position embedding came out as {tuple(patch.shape[-2:])} for a {h} x {w} grid")
    return torch.cat((pe[0, :1], patch.permute(0, 2, 3, 1).reshape(-1, EMBED)), dim=0).contiguous()


def attention(qkv: torch.Tensor) -> torch.Tensor:
    """softmax(q k^T / 8) v per head: qkv [B, N, 3, 6, 64] (any shape with those B x N x 1152 floats per image, packed) -> [B, N, 384]."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() >= 3 and qkv.shape[0] >= 1 and qkv.shape[1] >= 1
            and qkv[0, 0].numel() == 3 * EMBED):
        raise RuntimeError("wg_fused_dino.attention: a float32 [B, N, 3, 6, 64] tensor on a HIP device is required (there is no CPU path)")
    qkv = qkv.detach().contiguous()
    B, N = int(qkv.shape[0]), int(qkv.shape[1])
    out = torch.empty((B, N, EMBED), device=qkv.device, dtype=torch.float32)
    with torch.cuda.device(qkv.device):
        _native._check(_lib.wg_dino_attention(qkv.data_ptr(), B, N, out.data_ptr(), _stream(qkv.device)), "wg_dino_attention")
    return out


class DinoFeatures:
    """The extractor of one backbone module.  `block`: the block whose normalised output is returned (default num_heads - 1, the one
    `_get_dino_cached` asks for)."""

    def __init__(self, backbone, block=None):
        self.backbone = backbone
        self.block = int(backbone.num_heads) - 1 if block is None else int(block)
        if not model_covered(backbone, self.block):
            raise RuntimeError("wg_fused_dino.DinoFeatures: this backbone is not the covered model (see the module docstring)")
        self._pack()

    # ------------------------------------------------------------------------------------------ weights
    def _current_stamp(self):
        """(data_ptr, _version) of every parameter object that was packed, and the three scalars the kernels and the position embedding depend
        on.  The parameter OBJECTS are those found at packing time (walking the module costs half a millisecond, more than a small call's
        kernels): `load_state_dict`, in-place edits, `.data = ...` and `module.to(...)` keep them and are seen; after putting a NEW Parameter
        object into the module, call `refresh()`."""
        bb = self.backbone
        return tuple((t.data_ptr(), t._version) for t in self._params) + \
            (float(bb.norm.eps), float(getattr(bb, "interpolate_offset", 0.0) or 0.0), bool(getattr(bb, "interpolate_antialias", False)))

    def _pack(self):
        bb = self.backbone
        self._params = list(_used_parameters(bb, self.block + 1))
        self._packed = [t.detach().contiguous() for t in self._params]   # contiguous float32 parameters: views, no copies; kept alive here
        self._device = self._params[0].device
        self._pos = {}       # (h, w) -> prepared position embedding
        it = iter(self._packed)
        a = self._args = Args()
        a.struct_size = C.sizeof(Args)
        a.num_blocks, a.eps = self.block + 1, float(bb.norm.eps)
        a.patch_w, a.patch_b = next(it).data_ptr(), next(it).data_ptr()
        next(it)   # pos_embed: the one prepared for the call's grid is handed over
        a.cls_token, a.reg_tokens = next(it).data_ptr(), next(it).data_ptr()
        for i in range(self.block + 1):
            for name in BLOCK_FIELDS:
                setattr(a.blocks[i], name, next(it).data_ptr())
        a.norm_w, a.norm_b = next(it).data_ptr(), next(it).data_ptr()
        self._stamp = self._current_stamp()

    def refresh(self):
        """Walk the module again: after a Parameter object was replaced, or a block swapped."""
        if not model_covered(self.backbone, self.block):
            raise RuntimeError("wg_fused_dino.DinoFeatures: the backbone has left the covered case since construction")
        self._pack()

    def _fresh(self):
        if self._stamp != self._current_stamp():
            self.refresh()

    def _pos_for(self, h, w):
        pos = self._pos.get((h, w))
        if pos is None:
            pos = self._pos[(h, w)] = prepare_pos_embed(self.backbone, h, w)
        return pos

    # ------------------------------------------------------------------------------------------ the covered case
    @staticmethod
    def _input_ok(x, device, masks=None) -> bool:
        if masks is not None or not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.device == device):
            return False
        B, Cn, H, W = x.shape
        if B < 1 or Cn != 3 or H < PATCH or W < PATCH or H % PATCH or W % PATCH:
            return False
        return _lib.wg_dino_scratch_floats(B, H // PATCH, W // PATCH) > 0 and B * 3 * H * W < 2**31 and B * HEADS <= 65535

    @staticmethod
    def covers(backbone, x, block=None, masks=None) -> bool:
        """Are this model and this tensor the covered case?  Walks the module (about half a millisecond)."""
        return model_covered(backbone, block) and DinoFeatures._input_ok(x, backbone.pos_embed.device, masks)

    def input_covered(self, x, masks=None) -> bool:
        """`covers` for this extractor's own backbone, without walking the module again: the tensor's checks and the parameters' stamp."""
        if not DinoFeatures._input_ok(x, self._device, masks):
            return False
        try:
            self._fresh()
        except RuntimeError:
            return False
        return DinoFeatures._input_ok(x, self._device, masks)

    def features(self, x: torch.Tensor, _guard_floats: int = 0, _gemm_tiling: int = 0):
        """[B, 3, H, W] -> [B, 384, H / 14, W / 14].  `_guard_floats` (tests): output and scratch are allocated with that many floats on either
        side, filled with a pattern, and returned as (features, output buffer, scratch buffer).  `_gemm_tiling` (tests): 1 or 2 runs every
        product in the 64 x 64 or the 128 x 128 tiling instead of the one its size would choose; no bit depends on it."""
        self._fresh()
        if not DinoFeatures._input_ok(x, self._device):
            raise RuntimeError("wg_fused_dino.DinoFeatures.features: this input is not covered (float32 [B, 3, H, W] on the backbone's HIP device, "
                               "H and W multiples of 14); there is no PyTorch path")
        x = x.detach().contiguous()
        B, _, H, W = (int(v) for v in x.shape)
        h, w = H // PATCH, W // PATCH
        dev = x.device
        g = int(_guard_floats)
        need = scratch_floats(B, h, w)
        n_out = B * EMBED * h * w
        if g:
            out_buf = torch.full((n_out + 2 * g,), 12345.0, device=dev, dtype=torch.float32)
            scratch = torch.full((need + 2 * g,), 12345.0, device=dev, dtype=torch.float32)
        else:
            out_buf = torch.empty((n_out,), device=dev, dtype=torch.float32)
            scratch = torch.empty((need,), device=dev, dtype=torch.float32)
        out = out_buf[g:g + n_out].view(B, EMBED, h, w)
        pos = self._pos_for(h, w)
        a = self._args
        a.B, a.H, a.W, a.gemm_tiling = B, H, W, int(_gemm_tiling)
        a.image, a.pos = x.data_ptr(), pos.data_ptr()
        a.scratch, a.scratch_floats, a.out, a.stream = scratch[g:].data_ptr(), need, out.data_ptr(), _stream(dev)
        with torch.cuda.device(dev):
            _native._check(_lib.wg_dino_features(C.byref(a)), "wg_dino_features")
        return (out, out_buf, scratch) if g else out

    def attention(self, qkv: torch.Tensor) -> torch.Tensor:
        return attention(qkv)
