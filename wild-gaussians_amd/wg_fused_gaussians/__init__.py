"""Fused Gaussian activations + 3-D filter -- opt-in replacement of GaussianModel.get_gaussians's arithmetic
(wildgaussians/method.py:1060-1086).

    from wg_fused_gaussians import activate
    opacities, scales, rotations = activate(raw_opacities, raw_scales, raw_rotations, filter_3D)

with `raw_opacities` [P,1] logits, `raw_scales` [P,3] log-scales, `raw_rotations` [P,4] unnormalised quaternions and the
`filter_3D` [P,1] buffer; the results equal

    rotations = F.normalize(raw_rotations);  s = exp(raw_scales);  scales = sqrt(s^2 + filter_3D^2)
    opacities = sigmoid(raw_opacities) * sqrt(prod(s^2) / prod(s^2 + filter_3D^2))[:, None]

One HIP kernel forward, one backward (include/wg_activations.h, csrc/activations.hip); gradients flow to the three raw
parameters.  No CPU path: float32 tensors on a HIP device.

SURVEY.md 8f N4, the per-Gaussian bookkeeping after the backward pass (method.py:1995-1998, :1470-1477), in place, one kernel,
no host synchronisation (the torch code runs six boolean-mask index operations, each with a nonzero()):

    from wg_fused_gaussians import add_densification_stats
    add_densification_stats(radii, viewspace_points.grad, model.xyz_grad, model.denom, max_radii2D=model.max_radii2D,
                            xyz_gradient_accum_abs=model.xyz_gradient_accum_abs,
                            xyz_gradient_accum_abs_max=model.xyz_gradient_accum_abs_max)

GaussianModel.compute_3D_filter (method.py:1140-1190: a Python loop over all training cameras) as one kernel over all (Gaussian,
camera) pairs (include/wg_filter3d.h):

    from wg_fused_gaussians import CameraTable, compute_3D_filter
    table = CameraTable(train_cameras)             # once: the training cameras do not change
    filter_3D = compute_3D_filter(model.xyz, table)   # [P, 1]

GaussianModel.densify_and_prune and reset_opacity (method.py:1249-1468) as one plan, one host read and one gather over all arrays, with an
exact quantile that has no 2^24-element limit (include/wg_densify_prune.h):

    from wg_fused_gaussians import densify_and_prune, reset_opacity, quantile
    res = densify_and_prune(tensors, adam_state, stats, max_grad=..., min_opacity=..., extent=..., percent_dense=...,
                            enable_size_pruning=..., use_abs_gradient=...)   # res.tensors, res.adam_state, res.stats, res.counts, res.Q, res.origin

The appearance MLP of EmbeddingModel.forward (method.py:874-900) as one float32-MFMA kernel forward and one backward that recomputes the hidden
activations and saves only its inputs (include/wg_appearance_mlp.h); no `cat`, the image's embedding as a shared [E] vector or per row:

    from wg_fused_gaussians import appearance_mlp, embedding_forward
    offset_mul = appearance_mlp((features[..., :3], gembedding), list(model.mlp.parameters()), shared=aembedding)   # [P, 6]
    toned = embedding_forward(model, gembedding, aembedding, features)                                              # EmbeddingModel.forward

The same operator over the rows that reach the image only, forward and backward, with the list built on the device from the rasterizer's
`radii` (no `nonzero`, no host synchronisation) and every value the bits of the dense operator on gathered inputs (include/wg_appearance_rows.h):

    from wg_fused_gaussians import VisibleRows, appearance_rows
    rows = VisibleRows.from_radii(radii)                      # or .from_mask(mask) / .from_index(index)
    rows = VisibleRows.from_camera(rasterizer, xyz, scales, rotations)   # the same list BEFORE the frame is rendered (projection-only pass)
    offset_mul = appearance_mlp((features[..., :3], gembedding), weights, shared=aembedding, rows=rows)             # [P, 6], zeros at unlisted rows
    with appearance_rows(rows): ...                           # the forward that apply_optins(appearance_mlp=True) swaps in uses the list

The optimizer step over the same list: only the Gaussians the frame reached are updated, every other row keeps parameter and moments
(include/wg_adam_rows.h; 3D-GS's sparse_adam, gsplat's SelectiveAdam):

    from wg_fused_gaussians import VisibleRowsAdam
    optimizer = VisibleRowsAdam.adopt(model.optimizer);  optimizer.visible(radii);  optimizer.step()

The toned precomputed colours of one image (method.py:1555, :1557, :890-900, :1592-1598) from its [E] appearance embedding in one kernel, with the
embedding's gradient alone coming back in one kernel and a finishing launch, over the visible rows only (include/wg_appearance_colour.h); and the
loop of optimize_embedding (method.py:1786-1815) around it:

    from wg_fused_gaussians import toned_colours, fit_appearance_embedding, RowList
    colours = toned_colours(features, gembedding, embedding, xyz, campos, weights, deg, rows=RowList(radii > 0))      # [P, 3]
    embedding, losses, mses = fit_appearance_embedding(rasterizer, xyz, opacities, scales, rotations, features, gembedding, weights, embedding0, gt_image)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import torch

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_vp, _i = C.c_void_p, C.c_int
_lib.wg_activations_forward.restype = _i
_lib.wg_activations_forward.argtypes = [_i] + [_vp] * 8
_lib.wg_activations_backward.restype = _i
_lib.wg_activations_backward.argtypes = [_i] + [_vp] * 11
_lib.wg_densification_stats.restype = _i
_lib.wg_densification_stats.argtypes = [_i] + [_vp] * 8


def _prep(t, cols, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"wg_fused_gaussians: {name} must be a float32 tensor on a HIP device (there is no CPU path)")
    if t.numel() % cols:
        raise RuntimeError(f"wg_fused_gaussians: {name} has {t.numel()} elements, not a multiple of {cols}")
    return t.contiguous()


class _Activate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw_opacities, raw_scales, raw_rotations, filter_3D):
        o, s, r, f = _prep(raw_opacities, 1, "raw_opacities"), _prep(raw_scales, 3, "raw_scales"), \
            _prep(raw_rotations, 4, "raw_rotations"), _prep(filter_3D, 1, "filter_3D")
        P = o.numel()
        if s.numel() != 3 * P or r.numel() != 4 * P or f.numel() != P:
            raise RuntimeError("wg_fused_gaussians: inconsistent numbers of Gaussians")
        rot, sc, op = torch.empty_like(r), torch.empty_like(s), torch.empty_like(o)
        stream = torch.cuda.current_stream(o.device).cuda_stream
        with torch.cuda.device(o.device):
            _native._check(_lib.wg_activations_forward(P, r.data_ptr(), s.data_ptr(), o.data_ptr(), f.data_ptr(), rot.data_ptr(),
                                                       sc.data_ptr(), op.data_ptr(), stream), "wg_activations_forward")
        ctx.save_for_backward(o, s, r, f)
        return op, sc, rot

    @staticmethod
    def backward(ctx, g_op, g_sc, g_rot):
        o, s, r, f = ctx.saved_tensors
        P = o.numel()
        go, gs, gr = torch.empty_like(o), torch.empty_like(s), torch.empty_like(r)
        ptr = lambda t: t.contiguous().data_ptr() if t is not None else None
        g_op, g_sc, g_rot = [None if t is None else t.contiguous() for t in (g_op, g_sc, g_rot)]
        stream = torch.cuda.current_stream(o.device).cuda_stream
        with torch.cuda.device(o.device):
            _native._check(_lib.wg_activations_backward(P, r.data_ptr(), s.data_ptr(), o.data_ptr(), f.data_ptr(), ptr(g_rot), ptr(g_sc),
                                                        ptr(g_op), gr.data_ptr(), gs.data_ptr(), go.data_ptr(), stream),
                           "wg_activations_backward")
        return go, gs, gr, None


def activate(raw_opacities, raw_scales, raw_rotations, filter_3D):
    """-> (opacities [like raw_opacities], scales [like raw_scales], rotations [like raw_rotations])."""
    return _Activate.apply(raw_opacities, raw_scales, raw_rotations, filter_3D)


def add_densification_stats(radii, viewspace_grad, xyz_grad, denom, max_radii2D=None, xyz_gradient_accum_abs=None,
                            xyz_gradient_accum_abs_max=None):
    """In place, for every Gaussian with radii > 0 (the loop's visibility_filter): xyz_grad += |grad[:, :2]|, denom += 1,
    max_radii2D = max(max_radii2D, radii) and, when the two GOF buffers are given, xyz_gradient_accum_abs += |grad[:, 2]|,
    xyz_gradient_accum_abs_max = max(., |grad[:, 2]|).  `radii` int32 [P], `viewspace_grad` float32 [P, 3], the rest float32 with
    P elements ([P] or [P, 1]), all contiguous on one HIP device.  (A NaN gradient does not propagate into the two max buffers.)"""
    P = radii.numel()
    if not (radii.is_cuda and radii.dtype == torch.int32 and radii.is_contiguous()):
        raise RuntimeError("wg_fused_gaussians: radii must be a contiguous int32 tensor on a HIP device (there is no CPU path)")
    if (xyz_gradient_accum_abs is None) != (xyz_gradient_accum_abs_max is None):
        raise RuntimeError("wg_fused_gaussians: pass both GOF buffers or neither")
    g = _prep(viewspace_grad, 3, "viewspace_grad")
    if g.numel() != 3 * P:
        raise RuntimeError("wg_fused_gaussians: viewspace_grad must be [P, 3]")
    bufs = []
    for name, t in (("xyz_grad", xyz_grad), ("xyz_gradient_accum_abs", xyz_gradient_accum_abs),
                    ("xyz_gradient_accum_abs_max", xyz_gradient_accum_abs_max), ("denom", denom), ("max_radii2D", max_radii2D)):
        if t is None:
            bufs.append(None)
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == P):
            raise RuntimeError(f"wg_fused_gaussians: {name} must be a contiguous float32 tensor of {P} elements on the HIP device")
        bufs.append(t.data_ptr())
    stream = torch.cuda.current_stream(radii.device).cuda_stream
    with torch.cuda.device(radii.device):
        _native._check(_lib.wg_densification_stats(P, radii.data_ptr(), g.data_ptr(), bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], stream),
                       "wg_densification_stats")


# ---- fused Adam (include/wg_adam.h, csrc/adam.hip) -------------------------------------------------------------
class _AdamTensor(C.Structure):
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("numel", C.c_size_t),
                ("beta2", C.c_float), ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float), ("step_size", C.c_float),
                ("bias_correction2_sqrt", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)]


_lib.wg_fused_adam.restype = _i
_lib.wg_fused_adam.argtypes = [_i, C.POINTER(_AdamTensor), _vp]


class FusedAdam(torch.optim.Adam):
    """``torch.optim.Adam`` as the reference builds it (wildgaussians/method.py:1030-1049: one parameter group per Gaussian attribute,
    per-group ``lr`` / ``weight_decay``, ``eps=1e-15``) with ``step()`` (method.py:2019) as ONE kernel launch over all parameters
    instead of torch's ~ten elementwise passes per tensor:

        torch.optim.Adam = wg_fused_gaussians.FusedAdam      # before the model builds its optimizer, or edit that one line

    It IS a ``torch.optim.Adam``: ``param_groups``, ``state`` (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter, the layout the
    reference's densification code edits in place: method.py:1094-1102, 1268-1278, 1284-1297, 1312-1328), ``state_dict`` /
    ``load_state_dict``, ``zero_grad`` and the learning-rate schedule (``param_group['lr'] = ...``, method.py:1206-1210) are
    inherited; a state dict moves freely between the two classes.  Parameters must be float32 on a HIP device (others, and any
    group with ``amsgrad`` / ``maximize``, raise: there is no silent fallback); parameters without a gradient are skipped, as torch
    does.  The update is torch's, operation for operation in float32 (include/wg_adam.h)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **kw):
        for k in ("amsgrad", "maximize", "capturable", "differentiable"):
            if kw.get(k):
                raise NotImplementedError(f"wg_fused_gaussians.FusedAdam: {k}=True is not implemented")
        kw.pop("foreach", None)
        kw.pop("fused", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False,
                         **{k: v for k, v in kw.items() if k in ("amsgrad", "maximize", "capturable", "differentiable")})

    @classmethod
    def adopt(cls, optimizer: torch.optim.Adam) -> "FusedAdam":
        """A FusedAdam over the SAME parameters, group options (``lr``, ``name``, ``weight_decay`` ...) and state tensors as an existing
        ``torch.optim.Adam`` -- for callers whose code constructs the optimizer itself (wg_integration.apply_optins)."""
        groups = [{k: v for k, v in g.items() if k not in ("foreach", "fused")} for g in optimizer.param_groups]
        new = cls(groups, **{k: optimizer.defaults[k] for k in ("lr", "betas", "eps", "weight_decay")})
        for p, st in optimizer.state.items():
            new.state[p] = st
        return new

    @torch.no_grad()
    def step(self, closure=None):
        return self._step_dense(closure)

    def _step_dense(self, closure):   # not `step` itself: torch wraps every class's `step` with its hooks, which a subclass must not run twice
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        by_device = {}
        for _, p, d, g in self._descriptors():
            by_device.setdefault(p.device, []).append((d, g))   # g: keeps a contiguous copy alive until the launch is queued
        self._launch_dense(by_device)
        return loss

    @staticmethod
    def _launch_dense(by_device):
        for dev, items in by_device.items():
            arr = (_AdamTensor * len(items))(*[d for d, _ in items])
            with torch.cuda.device(dev):
                _native._check(_lib.wg_fused_adam(len(items), arr, torch.cuda.current_stream(dev).cuda_stream), "wg_fused_adam")

    def _descriptors(self):
        """One step's bookkeeping for every parameter that has a gradient -- the checks, torch's lazy state, the step counter, the version
        counters -- -> [(group, parameter, its wg_adam_tensor, the contiguous gradient)] in group order.  Nothing is launched."""
        out = []
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise NotImplementedError("wg_fused_gaussians.FusedAdam: amsgrad / maximize / decoupled_weight_decay are not implemented")
            beta1, beta2 = group["betas"]
            if not (0.5 < beta1 < 1.0 and 0.0 <= beta2 < 1.0):
                raise NotImplementedError("wg_fused_gaussians.FusedAdam: betas outside (0.5, 1) x [0, 1) are not implemented")
            lr = float(group["lr"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("wg_fused_gaussians.FusedAdam does not support sparse gradients")
                if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("wg_fused_gaussians.FusedAdam: parameters must be contiguous float32 tensors on a HIP device "
                                       "(there is no CPU path)")
                st = self.state[p]
                if len(st) == 0:   # torch's lazy state initialisation (torch/optim/adam.py: _init_group)
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if torch.is_tensor(st["step"]):
                    st["step"] += 1   # in place: a host scalar (a state dict loaded from torch.optim.Adam keeps it that way)
                    step = float(st["step"])
                else:
                    st["step"] = step = st["step"] + 1
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous() and m.shape == p.shape and v.shape == p.shape
                        and m.dtype == torch.float32 and v.dtype == torch.float32 and m.device == p.device and v.device == p.device):
                    raise RuntimeError("wg_fused_gaussians.FusedAdam: exp_avg / exp_avg_sq must be contiguous float32 tensors shaped "
                                       "and placed like their parameter")
                g = g if g.is_contiguous() else g.contiguous()
                # the step's scalars in double precision, rounded once when they enter the struct -- as torch's Python computes them
                d = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), beta2, 1.0 - beta1, 1.0 - beta2,
                                lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5, float(group["eps"]), float(group["weight_decay"]))
                out.append((group, p, d, g))
                # the kernel writes p, m and v behind torch's back: say so, as an in-place torch op would (autograd's saved-tensor
                # checks and the rasterizer binding's geometry reuse both read the version counter)
                torch.autograd.graph.increment_version(p)
                torch.autograd.graph.increment_version(m)
                torch.autograd.graph.increment_version(v)
        return out


# ---- the same step over the rows a frame reached (include/wg_adam_rows.h, csrc/adam/adam_rows.hip) ---------------------------------------
class _AdamRowsTensor(C.Structure):   # wg_adam_rows_tensor
    _fields_ = [("t", _AdamTensor), ("width", C.c_int64)]


_lib.wg_adam_rows_step.restype = _i
_lib.wg_adam_rows_step.argtypes = [_i, C.POINTER(_AdamRowsTensor), C.c_int64, _vp, C.c_int64, _vp, _vp]


class VisibleRowsAdam(FusedAdam):
    """``FusedAdam`` whose ``step()`` updates, in the per-Gaussian groups, only the rows of a list: the Gaussians with ``radii > 0`` in the
    frame just rendered -- 3D-GS's ``sparse_adam`` / gsplat's ``SelectiveAdam`` (include/wg_adam_rows.h):

        optimizer = VisibleRowsAdam(groups, lr=0.0, eps=1e-15)        # or VisibleRowsAdam.adopt(an existing torch.optim.Adam)
        optimizer.visible(radii)                                       # the list for the NEXT step() only; or step(rows=...)
        optimizer.step()

    A listed row receives ``FusedAdam``'s update, bit for bit.  An unlisted row keeps its parameter AND both moments, whatever its gradient
    holds: dense Adam would decay the moments and move the parameter along them although the frame gave it a gradient of exactly zero, and
    a loss term that gives invisible Gaussians a non-zero gradient (a regulariser over all scales, say) is ignored for them.  Results
    differ from dense Adam by design.

    ``per_gaussian``: the ``name``s of the groups whose parameters are ``[P, ...]`` tensors of one Gaussian per row.  Every other group
    (per-image appearance embeddings, the MLP, the uncertainty head) and every group of a step without a list takes the dense kernel, in
    the same call of ``step()``.  The list is a ``VisibleRows`` or the rasterizer's int32 ``radii`` (compacted on the device by
    ``VisibleRows.from_radii`` when the step needs it; no host wait).  ``step()`` consumes the list: the next step without one is
    ``FusedAdam.step()``.  A per-Gaussian parameter whose row count differs from the list's raises before anything is launched (the stale
    list after a densification); one without a gradient is skipped before that check, as torch does -- after the caller's
    ``densify_and_prune`` replaced the parameters between ``backward()`` and ``step()`` the step is a no-op for them and the list is dropped.

    The step count: a parameter's ``step`` advances once per ``step()`` that hands it to a kernel, with or without a list, and the bias
    correction follows this GLOBAL count, as in gsplat's ``SelectiveAdam`` -- not a count per row.  (The list's length lives on the device;
    a step whose list turns out empty there still counts.)  ``row_steps`` / ``dense_steps`` count the steps taken with / without a list.
    It is still a ``torch.optim.Adam``: ``adopt``, the state layout, state dicts and the lr schedule are FusedAdam's."""

    PER_GAUSSIAN = ("xyz", "features_dc", "opacities", "scales", "rotations", "embeddings", "features_rest")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, per_gaussian=PER_GAUSSIAN, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self.per_gaussian = frozenset(per_gaussian)
        self.row_steps = 0
        self.dense_steps = 0
        self._pending_rows = None

    def visible(self, rows):
        """Hand over the list for the NEXT ``step()`` only: a ``VisibleRows``, an int32 ``radii`` tensor, or None to withdraw it."""
        if rows is not None and not isinstance(rows, VisibleRows):
            if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 1):
                raise RuntimeError("wg_fused_gaussians.VisibleRowsAdam: rows must be a VisibleRows or a 1-D int32 radii tensor on a HIP device")
            rows = rows.detach()
        self._pending_rows = rows

    @torch.no_grad()
    def step(self, closure=None, *, rows=None):
        if rows is not None:
            self.visible(rows)
        rows, self._pending_rows = self._pending_rows, None   # consumed, whatever happens below
        if rows is None:
            self.dense_steps += 1
            return self._step_dense(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        listed = rows.P if isinstance(rows, VisibleRows) else rows.numel()
        for group in self.param_groups:   # before any bookkeeping and any launch
            if group.get("name") not in self.per_gaussian:
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.dim() < 1 or (listed is not None and p.shape[0] != listed):
                    raise RuntimeError(f"wg_fused_gaussians.VisibleRowsAdam: the row list was built for {listed} rows, parameter "
                                       f"'{group.get('name')}' has {p.shape[0] if p.dim() else 'no'} -- a list from before a densification?")
                if p.device != (rows.index.device if isinstance(rows, VisibleRows) else rows.device):
                    raise RuntimeError("wg_fused_gaussians.VisibleRowsAdam: the row list and the parameters are on different devices")
                if listed is None:   # an explicit index list of unknown P: every per-Gaussian tensor must at least agree
                    listed = p.shape[0]
        dense, sparse = {}, []
        for group, p, d, g in self._descriptors():
            if group.get("name") in self.per_gaussian:
                sparse.append((_AdamRowsTensor(d, p.numel() // p.shape[0] if p.shape[0] else 1), g))
            else:
                dense.setdefault(p.device, []).append((d, g))
        if sparse:
            if not isinstance(rows, VisibleRows):
                rows = VisibleRows.from_radii(rows)
            arr = (_AdamRowsTensor * len(sparse))(*[d for d, _ in sparse])
            dev = rows.index.device
            with torch.cuda.device(dev):
                _native._check(_lib.wg_adam_rows_step(len(sparse), arr, listed, rows.index.data_ptr(), rows.M,
                                                      None if rows.count is None else rows.count.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream), "wg_adam_rows_step")
        self._launch_dense(dense)
        self.row_steps += 1
        return loss


# ---- fused eval_sh (include/wg_sh_eval.h, csrc/sh_eval.hip) ------------------------------------------------------
_lib.wg_eval_sh_forward.restype = _i
_lib.wg_eval_sh_forward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp]
_lib.wg_eval_sh_backward.restype = _i
_lib.wg_eval_sh_backward.argtypes = [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]


class _EvalSH(torch.autograd.Function):
    @staticmethod
    def forward(ctx, deg, sh, dirs):
        P, K = sh.shape[0], sh.shape[2]
        out = torch.empty((P, 3), device=sh.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(sh.device).cuda_stream
        with torch.cuda.device(sh.device):
            _native._check(_lib.wg_eval_sh_forward(P, deg, K, sh.data_ptr(), dirs.data_ptr(), out.data_ptr(), stream), "wg_eval_sh_forward")
        ctx.deg = deg
        ctx.save_for_backward(sh, dirs)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        sh, dirs = ctx.saved_tensors
        P, K = sh.shape[0], sh.shape[2]
        g = grad_out.contiguous()
        need_sh, need_dirs = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_sh or need_dirs):
            return None, None, None
        grad_sh = torch.empty_like(sh)   # written whole by the kernel (it is the cheaper of the two outputs to always produce)
        grad_dirs = torch.empty_like(dirs) if need_dirs else None
        stream = torch.cuda.current_stream(sh.device).cuda_stream
        with torch.cuda.device(sh.device):
            _native._check(_lib.wg_eval_sh_backward(P, ctx.deg, K, sh.data_ptr(), dirs.data_ptr(), g.data_ptr(), grad_sh.data_ptr(),
                                                    None if grad_dirs is None else grad_dirs.data_ptr(), stream), "wg_eval_sh_backward")
        return None, grad_sh if need_sh else None, grad_dirs


def eval_sh(deg, sh: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """The reference's ``eval_sh(deg, sh, dirs)`` (wildgaussians/method.py:493-548) for ``sh`` [..., 3, K] and ``dirs`` [..., 3], degrees
    0..3, as one kernel forward and one backward (gradients to ``sh`` and ``dirs``) instead of ~60 elementwise kernels over strided
    slices and, backward, a zero-fill + slice-add of a [..., 3, K] tensor per coefficient.  float32 on a HIP device; no CPU path."""
    deg = int(deg)
    if not 0 <= deg <= 3:
        raise NotImplementedError("wg_fused_gaussians.eval_sh: degrees 0..3 are implemented")
    if sh.shape[-2] != 3 or dirs.shape[-1] != 3 or sh.shape[:-2] != dirs.shape[:-1] or sh.shape[-1] < (deg + 1) ** 2:
        raise RuntimeError("wg_fused_gaussians.eval_sh: expected sh [..., 3, K >= (deg + 1)^2] and dirs [..., 3] with equal leading dimensions")
    for name, t in (("sh", sh), ("dirs", dirs)):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"wg_fused_gaussians.eval_sh: {name} must be a float32 tensor on a HIP device (there is no CPU path)")
    lead = sh.shape[:-2]
    out = _EvalSH.apply(deg, sh.reshape(-1, 3, sh.shape[-1]).contiguous(), dirs.reshape(-1, 3).contiguous())
    return out.reshape(*lead, 3)


# ---- fused computation of filter_3D (include/wg_filter3d.h, csrc/activations.hip) ---------------------------------
class _Filter3dCamera(C.Structure):   # wg_filter3d_camera
    _fields_ = [("w2c", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("width", C.c_float), ("height", C.c_float)]


_lib.wg_compute_3d_filter.restype = _i
_lib.wg_compute_3d_filter.argtypes = [_i, _vp, _i, _vp, C.c_float, _vp, _vp, _vp]


def pack_cameras(poses, intrinsics, image_sizes):
    """Host side of ``CameraTable``: -> (table, focal_length) with ``table`` a float32 [C, 16] array of ``wg_filter3d_camera`` records and
    ``focal_length`` the largest fx of all cameras (0.0 without cameras).  The world-to-camera transform is the reference's
    (wildgaussians/method.py:1152-1161): ``np.linalg.inv`` of the 4x4 pose in the pose's own dtype, then float32."""
    import numpy as np
    poses, intrinsics, image_sizes = np.asarray(poses), np.asarray(intrinsics), np.asarray(image_sizes)
    if poses.ndim == 2:   # one camera (Cameras[i])
        poses, intrinsics, image_sizes = poses[None], intrinsics[None], image_sizes[None]
    n = poses.shape[0]
    if poses.shape[1:] != (3, 4) or intrinsics.shape != (n, 4) or image_sizes.shape != (n, 2):
        raise RuntimeError("wg_fused_gaussians: expected poses [C, 3, 4], intrinsics [C, 4] and image_sizes [C, 2]")
    c2w = np.concatenate([poses, np.broadcast_to(np.array([[0, 0, 0, 1]], dtype=poses.dtype), (n, 1, 4))], axis=1)
    w2c = np.linalg.inv(c2w)   # one LAPACK solve per matrix, as in the reference's loop
    table = np.empty((n, 16), dtype=np.float32)
    table[:, :12] = w2c[:, :3, :].reshape(n, 12)
    table[:, 12:14] = intrinsics[:, :2]
    table[:, 14:16] = image_sizes
    assert table.shape[1] * table.itemsize == C.sizeof(_Filter3dCamera)
    return table, (float(np.float32(intrinsics[:, 0].max())) if n else 0.0)


class CameraTable:
    """The training cameras as ``compute_3D_filter`` reads them, built once (they do not change during a run): the device array of
    64-byte records, ``focal_length`` (the largest fx) and the call's 8-byte workspace.  ``cameras``: the reference's ``Cameras`` object
    (numpy attributes ``poses`` [C, 3, 4] camera-to-world, ``intrinsics`` [C, 4], ``image_sizes`` [C, 2]) or a tuple of those three
    arrays.  A table serves one stream at a time (the workspace is its own)."""

    def __init__(self, cameras, device=None):
        arrays = cameras if isinstance(cameras, (tuple, list)) else (cameras.poses, cameras.intrinsics, cameras.image_sizes)
        if len(arrays) != 3 or arrays[2] is None:
            raise RuntimeError("wg_fused_gaussians: CameraTable needs poses, intrinsics and image_sizes")
        self.cameras = cameras   # keeps the object alive: callers key tables by its identity
        self.host, self.focal_length = pack_cameras(*arrays)
        self.num_cameras = self.host.shape[0]
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("wg_fused_gaussians: a CameraTable lives on a HIP device (there is no CPU path)")
        self.table = torch.from_numpy(self.host).to(self.device)
        self.workspace = torch.empty(8, dtype=torch.uint8, device=self.device)


@torch.no_grad()
def compute_3D_filter(xyz, cameras, out=None):
    """``GaussianModel.compute_3D_filter`` (wildgaussians/method.py:1140-1190) as one kernel over all (Gaussian, camera) pairs + one for
    the fill and the scale, stream-ordered, without a host synchronisation: -> ``filter_3D`` [P, 1] float32 (``out`` when given, written
    in place).  ``xyz`` [P, 3] float32 on a HIP device; ``cameras``: a ``CameraTable`` (build it once) or anything one can be built from
    (then built per call).  Where no camera sees any point (the reference raises) every value is 100000 / focal_length * sqrt(0.2)."""
    if not (torch.is_tensor(xyz) and xyz.is_cuda and xyz.dtype == torch.float32):
        raise RuntimeError("wg_fused_gaussians: xyz must be a float32 tensor on a HIP device (there is no CPU path)")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError("wg_fused_gaussians: xyz must be [P, 3]")
    table = cameras if isinstance(cameras, CameraTable) else CameraTable(cameras, device=xyz.device)
    if table.device != xyz.device:
        raise RuntimeError("wg_fused_gaussians: the CameraTable and xyz are on different devices")
    x = xyz.detach().contiguous()
    P = x.shape[0]
    if out is None:
        out = torch.empty((P, 1), device=x.device, dtype=torch.float32)
    else:
        if not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == P):
            raise RuntimeError(f"wg_fused_gaussians: out must be a contiguous float32 tensor of {P} elements on xyz's device")
        torch.autograd.graph.increment_version(out)   # written behind torch's back (as FusedAdam says it: the binding's geometry reuse reads it)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        _native._check(_lib.wg_compute_3d_filter(P, x.data_ptr(), table.num_cameras, table.table.data_ptr() if table.num_cameras else None,
                                                 table.focal_length, out.data_ptr(), table.workspace.data_ptr(), stream),
                       "wg_compute_3d_filter")
    return out.view(P, 1)


# ---- fused densify-and-prune, exact quantile, reset_opacity (include/wg_densify_prune.h, csrc/densify.hip) -------------------------
class _DensifyParams(C.Structure):   # wg_densify_params
    _fields_ = [("max_grad", C.c_float), ("min_opacity", C.c_float), ("dense_threshold", C.c_float), ("size_threshold", C.c_float),
                ("enable_size_pruning", C.c_int32), ("use_abs_gradient", C.c_int32)]


class _DensifyCounts(C.Structure):   # wg_densify_counts
    _fields_ = [("n_out", C.c_int64 * 4), ("n_cloned", C.c_int64), ("n_split", C.c_int64), ("n_pruned", C.c_int64), ("n_hot", C.c_int64),
                ("ratio", C.c_float), ("Q", C.c_float), ("reserved", C.c_int32 * 2)]


class _DensifyArray(C.Structure):   # wg_densify_array
    _fields_ = [("src", _vp), ("dst", _vp), ("row_floats", C.c_int32), ("role", C.c_int32)]


_DP_COPY, _DP_ZERO_NEW, _DP_XYZ, _DP_SCALES = 0, 1, 2, 3
_DP_MAX_ARRAYS = 48
_lib.wg_densify_scratch_bytes.restype = C.c_size_t
_lib.wg_densify_scratch_bytes.argtypes = [C.c_int64]
_lib.wg_quantile.restype = _i
_lib.wg_quantile.argtypes = [C.c_int64, _vp, C.c_double, _vp, _vp, _vp]
_lib.wg_densify_plan.restype = _i
_lib.wg_densify_plan.argtypes = [C.c_int64, C.POINTER(_DensifyParams)] + [_vp] * 8
_lib.wg_densify_apply.restype = _i
_lib.wg_densify_apply.argtypes = [C.c_int64, C.POINTER(_DensifyCounts), _vp, _i, C.POINTER(_DensifyArray)] + [_vp] * 6
_lib.wg_reset_opacity.restype = _i
_lib.wg_reset_opacity.argtypes = [C.c_int64] + [_vp] * 7


def _no_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"wg_fused_gaussians.{what} is not supported inside a stream capture: the output size is data-dependent")


def _rows(t, P, name):
    """A contiguous float32 HIP tensor whose leading dimension is the P Gaussians."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"wg_fused_gaussians: {name} must be a float32 tensor on a HIP device (there is no CPU path)")
    if t.dim() < 1 or t.shape[0] != P:
        raise RuntimeError(f"wg_fused_gaussians: {name} must have {P} rows")
    return t.detach().contiguous()


@torch.no_grad()
def quantile(values, q):
    """``torch.quantile(values.reshape(-1), q)`` (linear interpolation) by an exact radix selection, without torch's limit of 2^24 elements:
    -> a 0-dim float32 tensor on the device, no host synchronisation.  Above 2^24 elements the rank is formed in float64
    (include/wg_densify_prune.h).  NaN-free float32 values on a HIP device."""
    if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32):
        raise RuntimeError("wg_fused_gaussians: values must be a float32 tensor on a HIP device (there is no CPU path)")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise RuntimeError("wg_fused_gaussians: quantile() q must be in [0, 1]")
    v = values.detach().contiguous().reshape(-1)
    if v.numel() == 0:
        raise RuntimeError("wg_fused_gaussians: quantile() of an empty tensor")
    out = torch.empty((), device=v.device, dtype=torch.float32)
    scratch = torch.empty(_lib.wg_densify_scratch_bytes(0), device=v.device, dtype=torch.uint8)
    with torch.cuda.device(v.device):
        _native._check(_lib.wg_quantile(v.numel(), v.data_ptr(), q, out.data_ptr(), scratch.data_ptr(),
                                        torch.cuda.current_stream(v.device).cuda_stream), "wg_quantile")
    return out


class DensifyResult:
    """What ``densify_and_prune`` returns: ``tensors`` / ``adam_state`` / ``stats`` (dicts shaped like the inputs, P_new rows), ``counts`` =
    (n_cloned, n_split_parents, n_pruned) as the reference returns them, ``Q`` (None without use_abs_gradient) and ``ratio`` (floats),
    ``n_hot``, ``n_out`` (rows per kind) and ``origin`` (int32 [P_new, 2]: source index, kind 0 original / 1 clone / 2, 3 children)."""
    __slots__ = ("tensors", "adam_state", "stats", "counts", "Q", "ratio", "n_hot", "n_out", "origin", "noise")


@torch.no_grad()
def densify_and_prune(tensors, adam_state, stats, *, max_grad, min_opacity, extent, percent_dense, enable_size_pruning, use_abs_gradient,
                      noise=None, generator=None):
    """``GaussianModel.densify_and_prune`` (wildgaussians/method.py:1280-1468) in one GPU pass: a plan (decisions, exact quantile, offsets),
    ONE host wait for the new count, and one gather that moves every array once.

    ``tensors``: name -> [P, ...] raw parameter; "xyz", "scales", "rotations" and "opacities" are required, everything else is copied.
    ``adam_state``: name -> (exp_avg, exp_avg_sq) or a dict holding those two keys (torch's optimizer state) or None; copied for surviving
    originals, zero for new rows.  ``stats``: name -> per-Gaussian buffer ([P] or [P, 1]); "xyz_grad", "denom" and, with use_abs_gradient,
    "xyz_gradient_accum_abs" drive the decisions; all are carried like the moments (the reference does not reset them).
    ``noise``: the [2 S, 3] standard-normal draw of the split, copy-major; None: ``torch.randn`` on the device with ``generator``, drawn
    after S is known.  Inputs are left untouched.  -> ``DensifyResult``."""
    for k in ("xyz", "scales", "rotations", "opacities"):
        if k not in tensors:
            raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: tensors[{k!r}] is required")
    for k in ("xyz_grad", "denom") + (("xyz_gradient_accum_abs",) if use_abs_gradient else ()):
        if stats.get(k) is None:
            raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: stats[{k!r}] is required")
    P = tensors["xyz"].shape[0]
    dev = tensors["xyz"].device
    src = {k: _rows(t, P, k) for k, t in tensors.items()}
    _no_capture("densify_and_prune")
    for k, cols in (("xyz", 3), ("scales", 3), ("rotations", 4), ("opacities", 1)):
        if src[k].numel() != P * cols:
            raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: {k} must be [P, {cols}]")
    moments = {}
    for k, st in (adam_state or {}).items():
        if st is None or k not in src:
            continue
        m, v = (st["exp_avg"], st["exp_avg_sq"]) if isinstance(st, dict) else st
        m, v = _rows(m, P, k + ".exp_avg"), _rows(v, P, k + ".exp_avg_sq")
        if m.shape != src[k].shape or v.shape != src[k].shape:
            raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: the moments of {k} must be shaped like it")
        moments[k] = (m, v)
    bufs = {k: _rows(t, P, k) for k, t in stats.items() if t is not None}
    for k, t in bufs.items():
        if t.numel() != P:
            raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: stats[{k!r}] must hold one float per Gaussian")
    if any(t.device != dev for t in list(src.values()) + list(bufs.values()) + [x for mv in moments.values() for x in mv]):
        raise RuntimeError("wg_fused_gaussians.densify_and_prune: all tensors must be on one device")
    # thresholds as the reference's comparisons see them: Python forms the products in double, the float32 tensor meets them as float32
    prm = _DensifyParams(float(max_grad), float(min_opacity), float(percent_dense) * float(extent), 0.1 * float(extent),
                         int(bool(enable_size_pruning)), int(bool(use_abs_gradient)))
    scratch = torch.empty(max(_lib.wg_densify_scratch_bytes(P), 1), device=dev, dtype=torch.uint8)
    mailbox = torch.zeros(C.sizeof(_DensifyCounts), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev):
        _native._check(_lib.wg_densify_plan(P, C.byref(prm), bufs["xyz_grad"].data_ptr(), bufs["denom"].data_ptr(),
                                            bufs["xyz_gradient_accum_abs"].data_ptr() if use_abs_gradient else None,
                                            src["scales"].data_ptr(), src["opacities"].data_ptr(), scratch.data_ptr(), mailbox.data_ptr(),
                                            stream.cuda_stream), "wg_densify_plan")
        stream.synchronize()   # the call's only host wait: the new count
        counts = _DensifyCounts.from_buffer_copy(mailbox.numpy().tobytes())
        n_out = [int(x) for x in counts.n_out]
        n_new, S = sum(n_out), int(counts.n_split)
        if noise is None:
            noise = torch.randn((2 * S, 3), device=dev, dtype=torch.float32, generator=generator)
        else:
            if not (torch.is_tensor(noise) and noise.is_cuda and noise.dtype == torch.float32 and tuple(noise.shape) == (2 * S, 3)):
                raise RuntimeError(f"wg_fused_gaussians.densify_and_prune: noise must be a float32 [{2 * S}, 3] tensor on the device "
                                   f"(2 x {S} split Gaussians)")
            noise = noise.contiguous()
        new = lambda t: torch.empty((n_new,) + tuple(t.shape[1:]), device=dev, dtype=torch.float32)  # noqa: E731
        res = DensifyResult()
        res.tensors = {k: new(t) for k, t in src.items()}
        res.adam_state = {k: (new(m), new(v)) for k, (m, v) in moments.items()}
        res.stats = {k: new(t) for k, t in bufs.items()}
        res.origin = torch.empty((n_new, 2), device=dev, dtype=torch.int32)
        table = []
        for k, t in src.items():
            role = _DP_XYZ if k == "xyz" else _DP_SCALES if k == "scales" else _DP_COPY
            table.append(_DensifyArray(t.data_ptr(), res.tensors[k].data_ptr(), t.numel() // max(P, 1), role))
            if k in moments:
                for s_, d_ in zip(moments[k], res.adam_state[k]):
                    table.append(_DensifyArray(s_.data_ptr(), d_.data_ptr(), t.numel() // max(P, 1), _DP_ZERO_NEW))
        for k, t in bufs.items():
            table.append(_DensifyArray(t.data_ptr(), res.stats[k].data_ptr(), 1, _DP_ZERO_NEW))
        if P and n_new:
            for lo in range(0, len(table), _DP_MAX_ARRAYS):   # one launch for up to 48 arrays (the reference's model has 27)
                part = table[lo:lo + _DP_MAX_ARRAYS]
                arr = (_DensifyArray * len(part))(*part)
                _native._check(_lib.wg_densify_apply(P, C.byref(counts), scratch.data_ptr(), len(part), arr, src["xyz"].data_ptr(),
                                                     src["scales"].data_ptr(), src["rotations"].data_ptr(), noise.data_ptr(),
                                                     res.origin.data_ptr(), stream.cuda_stream), "wg_densify_apply")
    res.counts = (int(counts.n_cloned), S, int(counts.n_pruned))
    res.Q = float(counts.Q) if use_abs_gradient else None
    res.ratio, res.n_hot, res.n_out, res.noise = float(counts.ratio), int(counts.n_hot), tuple(n_out), noise
    return res


@torch.no_grad()
def reset_opacity(opacities, scales, filter_3D, exp_avg=None, exp_avg_sq=None):
    """``GaussianModel.reset_opacity``'s arithmetic (wildgaussians/method.py:1252-1266) as one elementwise kernel: -> the new raw opacities
    (a new tensor shaped like ``opacities``); ``exp_avg`` / ``exp_avg_sq`` (the opacity moments), when given, are zeroed in place."""
    P = opacities.shape[0] if torch.is_tensor(opacities) and opacities.dim() else 0
    o, s, f = _rows(opacities, P, "opacities"), _rows(scales, P, "scales"), _rows(filter_3D, P, "filter_3D")
    if o.numel() != P or s.numel() != 3 * P or f.numel() != P:
        raise RuntimeError("wg_fused_gaussians.reset_opacity: expected opacities [P, 1], scales [P, 3] and filter_3D [P, 1]")
    for name, t in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t is not None:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == P and t.device == o.device):
                raise RuntimeError(f"wg_fused_gaussians.reset_opacity: {name} must be a contiguous float32 tensor of {P} elements on the device")
            torch.autograd.graph.increment_version(t)
    out = torch.empty_like(o)
    with torch.cuda.device(o.device):
        _native._check(_lib.wg_reset_opacity(P, o.data_ptr(), s.data_ptr(), f.data_ptr(), out.data_ptr(),
                                             None if exp_avg is None else exp_avg.data_ptr(),
                                             None if exp_avg_sq is None else exp_avg_sq.data_ptr(),
                                             torch.cuda.current_stream(o.device).cuda_stream), "wg_reset_opacity")
    return out


# ---- fused appearance MLP (include/wg_appearance_mlp.h, csrc/appearance/mlp.hip) ------------------------------------------------------
class _MlpSegment(C.Structure):   # wg_appearance_mlp_segment
    _fields_ = [("ptr", _vp), ("width", C.c_int32), ("reserved", C.c_int32), ("row_stride", C.c_int64)]


class _MlpArgs(C.Structure):   # wg_appearance_mlp_args
    _fields_ = [("struct_size", C.c_size_t), ("P", C.c_int64), ("num_segments", C.c_int32), ("shared_width", C.c_int32),
                ("segments", _MlpSegment * 3), ("shared", _vp),
                ("W1", _vp), ("b1", _vp), ("W2", _vp), ("b2", _vp), ("W3", _vp), ("b3", _vp),
                ("out_scale", C.c_float), ("max_workgroups", C.c_int32), ("out", _vp), ("dL_dout", _vp),
                ("grad_segment", _vp * 3), ("grad_row_stride", C.c_int64 * 3), ("grad_shared", _vp),
                ("dW1", _vp), ("db1", _vp), ("dW2", _vp), ("db2", _vp), ("dW3", _vp), ("db3", _vp),
                ("scratch", _vp), ("scratch_floats", C.c_int64), ("stream", _vp)]


_lib.wg_appearance_mlp_scratch_floats.restype = C.c_int64
_lib.wg_appearance_mlp_scratch_floats.argtypes = [C.c_int64, C.c_int32]
_lib.wg_appearance_mlp_forward.restype = _i
_lib.wg_appearance_mlp_forward.argtypes = [C.POINTER(_MlpArgs)]
_lib.wg_appearance_mlp_backward.restype = _i
_lib.wg_appearance_mlp_backward.argtypes = [C.POINTER(_MlpArgs)]
MLP_HIDDEN, MLP_OUT, MLP_MAX_WIDTH, MLP_TILE_ROWS = 128, 6, 64, 64
MLP_PARTIAL_FLOATS, MLP_SCRATCH_HEAD_FLOATS = 128 * 64 + 128 * 128 + 6 * 128 + 128 + 128 + 8, 128


def appearance_mlp_scratch_floats(P, max_workgroups=0):
    """Floats of scratch a backward call needs (max_workgroups = 0 asks the current device for its compute-unit count)."""
    return _native._check(_lib.wg_appearance_mlp_scratch_floats(int(P), int(max_workgroups)), "wg_appearance_mlp_scratch_floats")


def _mlp_row_view(t, name):
    """A [P, w] float32 device tensor the kernel can read in place: unit stride along the row, any row stride >= w."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= 1):
        raise RuntimeError(f"wg_fused_gaussians.appearance_mlp: {name} must be a [P, w] float32 tensor on a HIP device (there is no CPU path)")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _mlp_fill(args, inputs, shared, weights, out_scale, max_workgroups, stream):
    args.struct_size = C.sizeof(_MlpArgs)
    args.P = inputs[0].shape[0]
    args.num_segments = len(inputs)
    for i, t in enumerate(inputs):
        args.segments[i].ptr = t.data_ptr()
        args.segments[i].width = t.shape[1]
        args.segments[i].row_stride = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    args.shared_width = 0 if shared is None else shared.numel()
    args.shared = None if shared is None else shared.data_ptr()
    args.W1, args.b1, args.W2, args.b2, args.W3, args.b3 = [w.data_ptr() for w in weights]
    args.out_scale = out_scale
    args.max_workgroups = max_workgroups
    args.stream = stream


def _mlp_operands(n_inputs, tensors):
    """(inputs..., shared or None, W1 b1 W2 b2 W3 b3) as the autograd functions receive them -> checked and readable by the kernels:
    (inputs, shared, weights, P, device)."""
    inputs = [_mlp_row_view(t, f"inputs[{i}]") for i, t in enumerate(tensors[:n_inputs])]
    shared = tensors[n_inputs]
    weights = tensors[n_inputs + 1:]
    P = inputs[0].shape[0]
    dev = inputs[0].device
    Kr = sum(t.shape[1] for t in inputs)
    if any(t.shape[0] != P or t.device != dev for t in inputs):
        raise RuntimeError("wg_fused_gaussians.appearance_mlp: inputs must have the same number of rows, on one device")
    if shared is not None:
        if not (shared.is_cuda and shared.dtype == torch.float32 and shared.dim() == 1 and shared.device == dev):
            raise RuntimeError("wg_fused_gaussians.appearance_mlp: shared must be a 1-D float32 tensor on the inputs' device")
        shared = shared.contiguous()
    K = Kr + (0 if shared is None else shared.numel())
    shapes = [(MLP_HIDDEN, K), (MLP_HIDDEN,), (MLP_HIDDEN, MLP_HIDDEN), (MLP_HIDDEN,), (MLP_OUT, MLP_HIDDEN), (MLP_OUT,)]
    if len(weights) != 6 or any(not (w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == s and w.device == dev)
                                for w, s in zip(weights, shapes)):
        raise RuntimeError(f"wg_fused_gaussians.appearance_mlp: weights must be float32 (W1 b1 W2 b2 W3 b3) of shapes {shapes} on the "
                           "inputs' device")
    weights = [w.contiguous() for w in weights]
    return inputs, shared, weights, P, dev


class _AppearanceMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n_inputs, out_scale, max_workgroups, *tensors):
        inputs, shared, weights, P, dev = _mlp_operands(n_inputs, tensors)
        out = torch.empty((P, MLP_OUT), dtype=torch.float32, device=dev)
        args = _MlpArgs()
        _mlp_fill(args, inputs, shared, weights, out_scale, max_workgroups, torch.cuda.current_stream(dev).cuda_stream)
        args.out = out.data_ptr()
        with torch.cuda.device(dev):
            _native._check(_lib.wg_appearance_mlp_forward(C.byref(args)), "wg_appearance_mlp_forward")
        ctx.save_for_backward(*inputs, *([] if shared is None else [shared]), *weights)   # the inputs and nothing else
        ctx.n_inputs, ctx.has_shared, ctx.out_scale, ctx.max_workgroups = n_inputs, shared is not None, out_scale, max_workgroups
        return out

    @staticmethod
    def backward(ctx, g_out):
        saved = ctx.saved_tensors
        n = ctx.n_inputs
        inputs = list(saved[:n])
        shared = saved[n] if ctx.has_shared else None
        weights = list(saved[n + (1 if ctx.has_shared else 0):])
        need = ctx.needs_input_grad[3:]
        need_in, need_sh, need_w = need[:n], need[n], any(need[n + 1:])
        P, dev = inputs[0].shape[0], inputs[0].device
        g_out = g_out.contiguous()
        args = _MlpArgs()
        _mlp_fill(args, inputs, shared, weights, ctx.out_scale, ctx.max_workgroups, torch.cuda.current_stream(dev).cuda_stream)
        args.dL_dout = g_out.data_ptr()
        g_in = [torch.empty((P, t.shape[1]), dtype=torch.float32, device=dev) if nd else None for t, nd in zip(inputs, need_in)]
        for i, g in enumerate(g_in):
            if g is not None:
                args.grad_segment[i] = g.data_ptr()
                args.grad_row_stride[i] = g.shape[1]
        g_sh = torch.empty_like(shared) if (shared is not None and need_sh) else None
        if g_sh is not None:
            args.grad_shared = g_sh.data_ptr()
        g_w = [torch.empty_like(w) for w in weights] if need_w else [None] * 6
        if need_w:
            args.dW1, args.db1, args.dW2, args.db2, args.dW3, args.db3 = [g.data_ptr() for g in g_w]
        with torch.cuda.device(dev):
            floats = appearance_mlp_scratch_floats(P, ctx.max_workgroups)
            scratch = torch.empty(floats, dtype=torch.float32, device=dev)
            args.scratch, args.scratch_floats = scratch.data_ptr(), floats
            _native._check(_lib.wg_appearance_mlp_backward(C.byref(args)), "wg_appearance_mlp_backward")
        g_w = [g if nd else None for g, nd in zip(g_w, need[n + 1:])]
        return (None, None, None, *g_in, g_sh, *g_w)


# ---- the same operator over a list of rows (include/wg_appearance_rows.h, csrc/appearance/rows.hip) -------------------------------------
class _RowsArgs(C.Structure):   # wg_appearance_rows_args
    _fields_ = [("struct_size", C.c_size_t), ("mlp", _MlpArgs), ("rows", _vp), ("M", C.c_int64), ("rows_count", _vp)]


_lib.wg_appearance_rows_scratch_floats.restype = C.c_int64
_lib.wg_appearance_rows_scratch_floats.argtypes = [C.c_int64, C.c_int32]
_lib.wg_appearance_rows_forward.restype = _i
_lib.wg_appearance_rows_forward.argtypes = [C.POINTER(_RowsArgs)]
_lib.wg_appearance_rows_backward.restype = _i
_lib.wg_appearance_rows_backward.argtypes = [C.POINTER(_RowsArgs)]
_lib.wg_appearance_rows_compact_scratch_bytes.restype = C.c_int64
_lib.wg_appearance_rows_compact_scratch_bytes.argtypes = [C.c_int64]
_lib.wg_appearance_rows_compact.restype = _i
_lib.wg_appearance_rows_compact.argtypes = [C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]
ROWS_COMPACT_BLOCK = 2048


def appearance_rows_scratch_floats(capacity, max_workgroups=0):
    """Floats of scratch a backward call over a list of this capacity needs (max_workgroups = 0 asks the current device)."""
    return _native._check(_lib.wg_appearance_rows_scratch_floats(int(capacity), int(max_workgroups)), "wg_appearance_rows_scratch_floats")


class VisibleRows:
    """The rows `appearance_mlp(rows=)` evaluates: `index` (int32 on the device), `M` (a host number: the exact entry count, or the
    capacity when `count` is given), `count` (None, or one int32 on the device: the real count) and `P` (the row count of the tensors the
    list belongs to; None when unknown).  `from_radii` and `from_mask` build the list on the device in ascending order with NO host
    synchronisation (include/wg_appearance_rows.h): the count stays on the device and M is the capacity P.  `from_camera` computes the
    radii itself, before the frame is rendered, and keeps them in `radii` (None in every other list)."""
    __slots__ = ("index", "M", "count", "P", "radii")

    def __init__(self, index, M, count=None, P=None):
        if index.numel() == 0:   # the C-ABI refuses a null list; an empty one still has an address
            index = torch.zeros(1, dtype=torch.int32, device=index.device)
        self.index, self.M, self.count, self.P = index, int(M), count, (None if P is None else int(P))
        self.radii = None

    @staticmethod
    def _compact(flags, is_radii):
        P = flags.numel()
        dev = flags.device
        index = torch.empty(P, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            nbytes = _native._check(_lib.wg_appearance_rows_compact_scratch_bytes(P), "wg_appearance_rows_compact_scratch_bytes")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ptr = flags.data_ptr() if P else None
            _native._check(_lib.wg_appearance_rows_compact(P, ptr if is_radii else None, None if is_radii else ptr, index.data_ptr() if P else None,
                                                           count.data_ptr(), scratch.data_ptr(), nbytes,
                                                           torch.cuda.current_stream(dev).cuda_stream), "wg_appearance_rows_compact")
        return VisibleRows(index, P, count, P)

    @classmethod
    def from_radii(cls, radii):
        """Rows with radii > 0 (`radii`: the rasterizer's int32 [P])."""
        if not (torch.is_tensor(radii) and radii.is_cuda and radii.dtype == torch.int32 and radii.dim() == 1):
            raise RuntimeError("wg_fused_gaussians.VisibleRows.from_radii: radii must be a 1-D int32 tensor on a HIP device")
        return cls._compact(radii.detach().contiguous(), True)

    @classmethod
    def from_camera(cls, rasterizer, means3D, scales=None, rotations=None, cov3D_precomp=None, *, filter_3D=None, opacities=None):
        """The rows that reach the image of `rasterizer`'s camera, BEFORE the frame is rendered: the projection-only pass
        (`GaussianRasterizer.project_radii`, same arguments: include/wg_rasterizer.h, wg_project_radii), then `from_radii`'s compaction -- four
        launches on the current stream, no host synchronisation, the count stays on the device.  The radii are the bits the forward call will
        write, so the list is the one `from_radii(radii_of_the_forward_call)` builds; they are kept in `.radii`.  With it the step can run the
        appearance MLP over the visible rows only AND render the raw and the toned image in one `sh_second=True` call (INTEGRATION.md
        section 5)."""
        radii = rasterizer.project_radii(means3D, scales, rotations, cov3D_precomp, filter_3D=filter_3D, opacities=opacities)
        rows = cls._compact(radii, True)
        rows.radii = radii
        return rows

    @classmethod
    def from_mask(cls, mask):
        """Rows whose mask byte is non-zero (`mask`: bool or uint8 [P]; a bool mask is viewed as uint8, not copied)."""
        if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype in (torch.bool, torch.uint8) and mask.dim() == 1):
            raise RuntimeError("wg_fused_gaussians.VisibleRows.from_mask: mask must be a 1-D bool or uint8 tensor on a HIP device")
        mask = mask.detach().contiguous()
        return cls._compact(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, False)

    @classmethod
    def from_index(cls, index, P=None):
        """An explicit list of row indices (int32 or int64, on the device), in any order; M is its length, a host number."""
        if not (torch.is_tensor(index) and index.is_cuda and index.dtype in (torch.int32, torch.int64) and index.dim() == 1):
            raise RuntimeError("wg_fused_gaussians.VisibleRows.from_index: index must be a 1-D int32 / int64 tensor on a HIP device")
        return cls(index.detach().to(torch.int32).contiguous(), index.numel(), None, P)


def _rows_fill(args, rows):
    args.struct_size = C.sizeof(_RowsArgs)
    args.rows = rows.index.data_ptr()
    args.M = rows.M
    args.rows_count = None if rows.count is None else rows.count.data_ptr()


class _AppearanceMlpRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n_inputs, out_scale, max_workgroups, rows, *tensors):
        inputs, shared, weights, P, dev = _mlp_operands(n_inputs, tensors)
        if rows.index.device != dev or (rows.count is not None and rows.count.device != dev) or rows.M > rows.index.numel():
            raise RuntimeError("wg_fused_gaussians.appearance_mlp: rows must be on the inputs' device and hold M entries")
        if rows.P is not None and rows.P != P:
            raise RuntimeError(f"wg_fused_gaussians.appearance_mlp: the row list was built for {rows.P} rows, the inputs have {P}")
        out = torch.zeros((P, MLP_OUT), dtype=torch.float32, device=dev)   # unlisted rows stay zero: the kernel writes listed rows only
        args = _RowsArgs()
        _mlp_fill(args.mlp, inputs, shared, weights, out_scale, max_workgroups, torch.cuda.current_stream(dev).cuda_stream)
        _rows_fill(args, rows)
        args.mlp.out = out.data_ptr()
        with torch.cuda.device(dev):
            _native._check(_lib.wg_appearance_rows_forward(C.byref(args)), "wg_appearance_rows_forward")
        ctx.save_for_backward(*inputs, *([] if shared is None else [shared]), *weights)   # the inputs (and the list) and nothing else
        ctx.rows = rows
        ctx.n_inputs, ctx.has_shared, ctx.out_scale, ctx.max_workgroups = n_inputs, shared is not None, out_scale, max_workgroups
        return out

    @staticmethod
    def backward(ctx, g_out):
        saved = ctx.saved_tensors
        n = ctx.n_inputs
        inputs = list(saved[:n])
        shared = saved[n] if ctx.has_shared else None
        weights = list(saved[n + (1 if ctx.has_shared else 0):])
        need = ctx.needs_input_grad[4:]
        need_in, need_sh, need_w = need[:n], need[n], any(need[n + 1:])
        P, dev = inputs[0].shape[0], inputs[0].device
        g_out = g_out.contiguous()
        args = _RowsArgs()
        _mlp_fill(args.mlp, inputs, shared, weights, ctx.out_scale, ctx.max_workgroups, torch.cuda.current_stream(dev).cuda_stream)
        _rows_fill(args, ctx.rows)
        m = args.mlp
        m.dL_dout = g_out.data_ptr()
        g_in = [torch.zeros((P, t.shape[1]), dtype=torch.float32, device=dev) if nd else None for t, nd in zip(inputs, need_in)]
        for i, g in enumerate(g_in):
            if g is not None:
                m.grad_segment[i] = g.data_ptr()
                m.grad_row_stride[i] = g.shape[1]
        g_sh = torch.empty_like(shared) if (shared is not None and need_sh) else None
        if g_sh is not None:
            m.grad_shared = g_sh.data_ptr()
        g_w = [torch.empty_like(w) for w in weights] if need_w else [None] * 6
        if need_w:
            m.dW1, m.db1, m.dW2, m.db2, m.dW3, m.db3 = [g.data_ptr() for g in g_w]
        with torch.cuda.device(dev):
            floats = appearance_rows_scratch_floats(ctx.rows.M, ctx.max_workgroups)
            scratch = torch.empty(floats, dtype=torch.float32, device=dev)
            m.scratch, m.scratch_floats = scratch.data_ptr(), floats
            _native._check(_lib.wg_appearance_rows_backward(C.byref(args)), "wg_appearance_rows_backward")
        g_w = [g if nd else None for g, nd in zip(g_w, need[n + 1:])]
        return (None, None, None, None, *g_in, g_sh, *g_w)


def appearance_mlp(inputs, weights, shared=None, out_scale=0.01, max_workgroups=0, rows=None):
    """-> [P, 6] = out_scale * (W3 . relu(W2 . relu(W1 . cat(inputs..., shared) + b1) + b2) + b3), one HIP kernel in float32 on the matrix
    cores; nothing but the inputs is saved for the backward pass, which recomputes the hidden activations (include/wg_appearance_mlp.h).

    inputs   one to three [P, w_i] float32 tensors, read in place (a view with unit stride along the row and any row stride, such as
             `features[..., :3]`, is not copied); the widths sum to 1..64
    weights  (W1 [128, K], b1, W2 [128, 128], b2, W3 [6, 128], b3) as nn.Linear holds them, K = sum of widths (+ len(shared))
    shared   optional [E <= 64] vector that every row carries behind its own columns (the image's appearance embedding)
    rows     optional VisibleRows: only the listed rows are evaluated, forward and backward (include/wg_appearance_rows.h).  The result is
             [P, 6] with zeros at unlisted rows, input gradients are [P, w_i] with zeros at unlisted rows, and every value has the bits of
             this operator run on `x[rows]` with the cotangent `g[rows]`.  None: all rows, the dense kernels
    Gradients go to whichever of inputs / shared / weights require them.  Two calls on the same inputs give the same bits."""
    inputs = list(inputs)
    if not 1 <= len(inputs) <= 3:
        raise RuntimeError("wg_fused_gaussians.appearance_mlp: one to three inputs")
    if rows is None:
        return _AppearanceMlp.apply(len(inputs), float(out_scale), int(max_workgroups), *inputs, shared, *weights)
    if not isinstance(rows, VisibleRows):
        raise RuntimeError("wg_fused_gaussians.appearance_mlp: rows must be a VisibleRows (from_radii, from_mask or from_index)")
    return _AppearanceMlpRows.apply(len(inputs), float(out_scale), int(max_workgroups), rows, *inputs, shared, *weights)


_rows_context = threading.local()


def current_appearance_rows():
    """The VisibleRows of the innermost active `appearance_rows` block of this thread, or None."""
    stack = getattr(_rows_context, "stack", None)
    return stack[-1] if stack else None


@contextlib.contextmanager
def appearance_rows(rows):
    """While active (in this thread), the `EmbeddingModel.forward` that wg_integration.apply_optins(appearance_mlp=True) swaps in evaluates
    the listed rows only:

        with appearance_rows(VisibleRows.from_radii(radii)):
            colors_toned = self.appearance_mlp(...)

    Blocks nest; leaving one restores the list of the enclosing block (none by default).  `rows` may be None: the dense operator inside."""
    if rows is not None and not isinstance(rows, VisibleRows):
        raise RuntimeError("wg_fused_gaussians.appearance_rows: rows must be a VisibleRows or None")
    stack = getattr(_rows_context, "stack", None)
    if stack is None:
        stack = _rows_context.stack = []
    stack.append(rows)
    try:
        yield rows
    finally:
        stack.pop()


_SH_C0 = 0.28209479177387814


def _mlp_covered(module):
    """The module's weights if its `mlp` is Linear(K, 128)-ReLU-Linear(128, 128)-ReLU-Linear(128, 6), else None."""
    nn = torch.nn
    mlp = getattr(module, "mlp", None)
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 5:
        return None
    l1, r1, l2, r2, l3 = mlp
    if not (isinstance(l1, nn.Linear) and isinstance(l2, nn.Linear) and isinstance(l3, nn.Linear) and isinstance(r1, nn.ReLU)
            and isinstance(r2, nn.ReLU)):
        return None
    if (l1.out_features, l2.in_features, l2.out_features, l3.in_features, l3.out_features) != (128, 128, 128, 128, 6):
        return None
    if l1.bias is None or l2.bias is None or l3.bias is None:
        return None
    return (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)


def embedding_forward(module, gembedding, aembedding, color, viewdir=None, *, original_forward=None, max_workgroups=0, rows=None):
    """EmbeddingModel.forward (wildgaussians/method.py:890-900) around the fused operator: `color[..., :3]`, `gembedding` and `aembedding`
    are read in place (no `cat`); an `aembedding` of shape [E] is the shared path, one of shape [P, E] the per-row path.  Calls the fused
    operator does not cover -- CPU tensors, a dtype other than float32, appearance_model_sh = True, an `mlp` of another shape -- go to the
    module's own forward (`original_forward`, default type(module).forward): the caller's code, not a fallback of this library.
    rows: an optional VisibleRows; the MLP then runs over the listed rows only and the toned result is 0 at every other row (its `mul` and
    `offset` are), which is what a rasterizer call that culls those rows never reads.  A list built for another row count raises."""
    weights = _mlp_covered(module)
    tensors = (gembedding, aembedding, color)
    ok = (weights is not None and not getattr(getattr(module, "config", None), "appearance_model_sh", False)
          and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors + tuple(weights))
          and color.dim() == 2 and gembedding.dim() == 2 and aembedding.dim() in (1, 2) and color.shape[1] >= 3 and color.shape[1] % 3 == 0
          and weights[0].shape[1] == 3 + gembedding.shape[1] + aembedding.shape[-1] and 3 + gembedding.shape[1] <= MLP_MAX_WIDTH
          and aembedding.shape[-1] <= MLP_MAX_WIDTH
          and (aembedding.dim() == 1 or 3 + gembedding.shape[1] + aembedding.shape[1] <= MLP_MAX_WIDTH))
    if not ok:
        fwd = original_forward if original_forward is not None else type(module).forward
        return fwd(module, gembedding, aembedding, color, viewdir)
    input_color = color
    if rows is not None and rows.P is not None and rows.P != color.shape[0]:
        raise RuntimeError(f"wg_fused_gaussians.embedding_forward: the row list was built for {rows.P} rows, color has {color.shape[0]}")
    if aembedding.dim() == 1:
        om = appearance_mlp((color[..., :3], gembedding), weights, shared=aembedding, out_scale=0.01, max_workgroups=max_workgroups, rows=rows)
    else:
        om = appearance_mlp((color[..., :3], gembedding, aembedding), weights, out_scale=0.01, max_workgroups=max_workgroups, rows=rows)
    offset, mul = torch.split(om, [3, 3], dim=-1)
    offset = torch.cat((offset / _SH_C0, torch.zeros_like(input_color[..., 3:])), dim=-1)
    mul = mul.repeat(1, input_color.shape[-1] // 3)
    return input_color * mul + offset


# ---- fused toned colours (include/wg_appearance_colour.h, csrc/appearance/colour.hip) --------------------------------------------------
class _ColourArgs(C.Structure):   # wg_appearance_colour_args
    _fields_ = [("struct_size", C.c_size_t), ("P", C.c_int64), ("M", C.c_int64), ("rows", _vp),
                ("features", _vp), ("features_row_stride", C.c_int64), ("deg", C.c_int32), ("gembedding_width", C.c_int32),
                ("gembedding", _vp), ("gembedding_row_stride", C.c_int64), ("shared", _vp), ("shared_width", C.c_int32),
                ("max_workgroups", C.c_int32), ("xyz", _vp), ("xyz_row_stride", C.c_int64), ("campos", _vp),
                ("W1", _vp), ("b1", _vp), ("W2", _vp), ("b2", _vp), ("W3", _vp), ("b3", _vp),
                ("out_scale", C.c_float), ("pre_clamp_max", C.c_float), ("post_clamp_max", C.c_float), ("reserved", C.c_int32),
                ("colours", _vp), ("dL_dcolours", _vp), ("grad_shared", _vp), ("scratch", _vp), ("scratch_floats", C.c_int64),
                ("stream", _vp)]


_lib.wg_appearance_colour_scratch_floats.restype = C.c_int64
_lib.wg_appearance_colour_scratch_floats.argtypes = [C.c_int64, C.c_int32]
_lib.wg_appearance_colour_forward.restype = _i
_lib.wg_appearance_colour_forward.argtypes = [C.POINTER(_ColourArgs)]
_lib.wg_appearance_colour_backward.restype = _i
_lib.wg_appearance_colour_backward.argtypes = [C.POINTER(_ColourArgs)]
COLOUR_COEFFS, COLOUR_TILE_ROWS, COLOUR_PARTIAL_FLOATS = 48, 64, 128


def appearance_colour_scratch_floats(M, max_workgroups=0):
    """Floats of scratch a backward call over M listed rows needs (max_workgroups = 0 asks the current device for its compute-unit count)."""
    return _native._check(_lib.wg_appearance_colour_scratch_floats(int(M), int(max_workgroups)), "wg_appearance_colour_scratch_floats")


class RowList:
    """The rows `toned_colours` evaluates, converted once: `index` (int32 [M] on the device) and M as a host number.  Built from a [P] bool
    mask (one `nonzero`, the only host synchronisation) or from an integer index tensor (none); pass the object itself to later calls."""
    __slots__ = ("index", "M")

    def __init__(self, rows):
        if isinstance(rows, RowList):
            self.index, self.M = rows.index, rows.M
            return
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 1):
            raise RuntimeError("wg_fused_gaussians.toned_colours: rows must be a 1-D bool mask or integer index tensor on a HIP device")
        if rows.dtype == torch.bool:
            rows = rows.nonzero().reshape(-1)
        elif rows.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("wg_fused_gaussians.toned_colours: rows must be a bool mask or an int32 / int64 index tensor")
        self.index = rows.detach().to(torch.int32).contiguous()
        self.M = self.index.numel()


def _colour_row_view(t, width, name):
    """A [P, >= width] float32 device tensor the kernel reads in place: unit stride along the row, any row stride >= width."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= width):
        raise RuntimeError(f"wg_fused_gaussians.toned_colours: {name} must be a [P, >= {width}] float32 tensor on a HIP device (there is no CPU path)")
    if t.shape[1] and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        t = t.contiguous()
    return t


def _colour_fill(args, features, gemb, embedding, xyz, campos, index, M, weights, deg, pre, post, out_scale, max_workgroups, stream):
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else t.shape[1]   # noqa: E731
    args.struct_size = C.sizeof(_ColourArgs)
    args.P, args.M = features.shape[0], M
    args.rows = None if index is None else index.data_ptr()
    args.features, args.features_row_stride, args.deg = features.data_ptr(), stride(features), deg
    G = gemb.shape[1]
    args.gembedding_width = G
    args.gembedding, args.gembedding_row_stride = (gemb.data_ptr(), stride(gemb)) if G else (None, 0)
    args.shared, args.shared_width = embedding.data_ptr(), embedding.numel()
    args.max_workgroups = max_workgroups
    args.xyz, args.xyz_row_stride, args.campos = xyz.data_ptr(), stride(xyz), campos.data_ptr()
    args.W1, args.b1, args.W2, args.b2, args.W3, args.b3 = [w.data_ptr() for w in weights]
    args.out_scale, args.pre_clamp_max, args.post_clamp_max = out_scale, pre, post
    args.stream = stream


class _TonedColours(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embedding, features, gemb, xyz, campos, index, M, deg, pre, post, out_scale, max_workgroups, *weights):
        P, dev = features.shape[0], features.device
        colours = torch.empty((P, 3), dtype=torch.float32, device=dev) if index is None else torch.zeros((P, 3), dtype=torch.float32, device=dev)
        args = _ColourArgs()
        _colour_fill(args, features, gemb, embedding, xyz, campos, index, M, weights, deg, pre, post, out_scale, max_workgroups,
                     torch.cuda.current_stream(dev).cuda_stream)
        args.colours = colours.data_ptr()
        with torch.cuda.device(dev):
            _native._check(_lib.wg_appearance_colour_forward(C.byref(args)), "wg_appearance_colour_forward")
        ctx.save_for_backward(embedding, features, gemb, xyz, campos, *([] if index is None else [index]), *weights)   # the inputs and nothing else
        ctx.has_index, ctx.conf = index is not None, (M, deg, pre, post, out_scale, max_workgroups)
        return colours

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        embedding, features, gemb, xyz, campos = saved[:5]
        index = saved[5] if ctx.has_index else None
        weights = saved[6 if ctx.has_index else 5:]
        M, deg, pre, post, out_scale, max_workgroups = ctx.conf
        dev = features.device
        g = g.contiguous()
        grad = torch.empty_like(embedding)
        args = _ColourArgs()
        _colour_fill(args, features, gemb, embedding, xyz, campos, index, M, weights, deg, pre, post, out_scale, max_workgroups,
                     torch.cuda.current_stream(dev).cuda_stream)
        args.dL_dcolours, args.grad_shared = g.data_ptr(), grad.data_ptr()
        with torch.cuda.device(dev):
            floats = appearance_colour_scratch_floats(M, max_workgroups)
            scratch = torch.empty(max(floats, 1), dtype=torch.float32, device=dev)
            args.scratch, args.scratch_floats = scratch.data_ptr(), floats
            _native._check(_lib.wg_appearance_colour_backward(C.byref(args)), "wg_appearance_colour_backward")
        return (grad,) + (None,) * (11 + len(weights))


def toned_colours(features, gembedding, embedding, xyz, campos, weights, deg, *, rows=None, pre_clamp_max=1.0, post_clamp_max=1.0,
                  out_scale=0.01, max_workgroups=0):
    """-> [P, 3] precomputed colours of the reference's toned path (wildgaussians/method.py:1555, :1557, :890-900, :1592-1598) in ONE kernel:
    `clamp_max`, EmbeddingModel.forward with the image's `embedding` [E] shared by all rows, both clamps, `eval_sh` at the normalised
    `xyz - campos` and `clamp_min(. + 0.5, 0)` (include/wg_appearance_colour.h).  Differentiable with respect to `embedding` ONLY: its
    gradient comes from one kernel and a finishing launch, without any weight gradient, input gradient or [P, 48] tensor.  Any other tensor
    argument that requires a gradient raises.

    features    [P, >= 48] float32, coefficient-major (`features.view(P, 16, 3)`), read in place through its row stride
    gembedding  [P, G], 3 + G <= 64;  embedding [E <= 64];  xyz [P, >= 3];  campos [3] ON THE DEVICE (the call does not synchronise)
    weights     (W1 [128, 3 + G + E], b1, W2 [128, 128], b2, W3 [6, 128], b3) as nn.Linear holds them
    deg         the active SH degree, 0..3
    rows        None (all rows), a [P] bool mask, an integer index tensor, or a `RowList` built from either -- a mask costs one `nonzero`,
                so build the RowList once and pass it to every later call.  Rows not listed are 0 in the result and read nothing.
    A clamp bound of float("inf") means no clamp.  Two calls with the same max_workgroups give the same bits."""
    weights = list(weights)
    names = ["features", "gembedding", "xyz", "campos"] + [f"weights[{i}]" for i in range(len(weights))]
    for name, t in zip(names, [features, gembedding, xyz, campos] + weights):
        if torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"wg_fused_gaussians.toned_colours: only the embedding receives a gradient; {name} is a constant here: detach it")
    deg = int(deg)
    if not 0 <= deg <= 3:
        raise NotImplementedError("wg_fused_gaussians.toned_colours: degrees 0..3 are implemented")
    features = _colour_row_view(features, COLOUR_COEFFS, "features")
    gembedding = _colour_row_view(gembedding, 0, "gembedding")
    xyz = _colour_row_view(xyz, 3, "xyz")
    P, dev, G = features.shape[0], features.device, gembedding.shape[1]
    for name, t, n in (("embedding", embedding, None), ("campos", campos, 3)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.device == dev and (n is None or t.numel() == n)):
            raise RuntimeError(f"wg_fused_gaussians.toned_colours: {name} must be a 1-D float32 tensor on the features' device"
                               + ("" if n is None else f" with {n} elements"))
    E = embedding.numel()
    if gembedding.shape[0] != P or xyz.shape[0] != P or gembedding.device != dev or xyz.device != dev:
        raise RuntimeError("wg_fused_gaussians.toned_colours: features, gembedding and xyz must have the same number of rows, on one device")
    if not (1 <= E <= MLP_MAX_WIDTH and 3 + G <= MLP_MAX_WIDTH):
        raise RuntimeError("wg_fused_gaussians.toned_colours: 3 + G <= 64 and 1 <= E <= 64 are implemented")
    shapes = [(MLP_HIDDEN, 3 + G + E), (MLP_HIDDEN,), (MLP_HIDDEN, MLP_HIDDEN), (MLP_HIDDEN,), (MLP_OUT, MLP_HIDDEN), (MLP_OUT,)]
    if len(weights) != 6 or any(not (torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == s and w.device == dev)
                                for w, s in zip(weights, shapes)):
        raise RuntimeError(f"wg_fused_gaussians.toned_colours: weights must be float32 (W1 b1 W2 b2 W3 b3) of shapes {shapes} on the features' device")
    index, M = None, P
    if rows is not None:
        rl = rows if isinstance(rows, RowList) else RowList(rows)
        if rl.index.device != dev:
            raise RuntimeError("wg_fused_gaussians.toned_colours: rows must be on the features' device")
        index, M = rl.index, rl.M
    return _TonedColours.apply(embedding.contiguous(), features.detach(), gembedding.detach(), xyz.detach(), campos.detach().contiguous(), index, M, deg,
                               float(pre_clamp_max), float(post_clamp_max), float(out_scale), int(max_workgroups),
                               *[w.detach().contiguous() for w in weights])


class _ScaleGrad(torch.autograd.Function):   # the caller's scale_grads: the value unchanged, the cotangent multiplied
    @staticmethod
    def forward(ctx, image, scale):
        ctx.save_for_backward(scale)
        return image.view_as(image)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def fit_appearance_embedding(rasterizer, means3D, opacities, scales, rotations, features, gembedding, weights, embedding0, gt_image, *,
                             campos=None, deg=None, iters=128, lr=0.1, loss="dssim+l1", lambda_dssim=0.2, grad_scale=None,
                             pre_clamp_max=1.0, post_clamp_max=1.0, max_workgroups=0, fixed_order=False):
    """The loop of WildGaussians.optimize_embedding (wildgaussians/method.py:1786-1815) at tensor level: `iters` Adam steps on the one [E]
    appearance embedding of a test image, geometry and camera frozen.  -> (embedding [E] on the device, losses [iters], mses [iters] on the
    host).

    Once: one forward call of `rasterizer` finds the Gaussians that reach the image (`radii > 0`) and their RowList.  Each step:
    `toned_colours(rows=...)`, `rasterizer(colors_precomp=...)` inside `colour_gradients_only(True)`, the loss ("dssim+l1":
    wg_fused_ssim.l1_ssim_loss with `lambda_dssim`; "mse"), `torch.optim.Adam(lr=lr)`.  `grad_scale` (the caller's scale_grads masks,
    multiplied together; broadcastable to the image) multiplies the image's cotangent and leaves its value unchanged.  The per-step losses
    stay on the device; the host reads them once, at the end.  `campos` / `deg` default to the rasterizer's settings.
    `fixed_order=True`: the loop runs inside `colour_gradients_only("fixed_order")` -- the colour-only backward pass without float atomics.
    Every other link of a step is reproducible already, so two calls then return the same embedding, losses and MSEs bit for bit."""
    from diff_gaussian_rasterization import colour_gradients_only
    from wg_fused_ssim import l1_ssim_loss
    if loss not in ("dssim+l1", "mse"):
        raise ValueError(f"Unknown appearance optimization type {loss}")
    rs = rasterizer.raster_settings
    campos = rs.campos if campos is None else campos
    deg = int(rs.sh_degree if deg is None else deg)
    consts = [t.detach() for t in (means3D, opacities, scales, rotations, features, gembedding, campos, gt_image)]
    means3D, opacities, scales, rotations, features, gembedding, campos, gt_image = consts
    weights = [w.detach() for w in weights]
    campos = campos.to(device=means3D.device, dtype=torch.float32).reshape(3)
    means2D = torch.zeros_like(means3D)
    with torch.no_grad():
        radii = rasterizer(means3D=means3D, means2D=means2D, opacities=opacities, colors_precomp=torch.zeros_like(means3D), scales=scales,
                           rotations=rotations)[1]
    rows = RowList(radii > 0)
    param = torch.nn.Parameter(embedding0.detach().clone().float())
    optimizer = torch.optim.Adam([param], lr=lr)
    iters = int(iters)
    record = torch.zeros((2, max(iters, 1)), dtype=torch.float32, device=means3D.device)
    with torch.enable_grad(), colour_gradients_only("fixed_order" if fixed_order else True):
        for i in range(iters):
            optimizer.zero_grad()
            colours = toned_colours(features, gembedding, param, means3D, campos, weights, deg, rows=rows, pre_clamp_max=pre_clamp_max,
                                    post_clamp_max=post_clamp_max, max_workgroups=max_workgroups)
            image = rasterizer(means3D=means3D, means2D=means2D, opacities=opacities, colors_precomp=colours, scales=scales, rotations=rotations)[0]
            if grad_scale is not None:
                image = _ScaleGrad.apply(image, grad_scale)
            if loss == "mse":
                value = mse = torch.nn.functional.mse_loss(image, gt_image)
            else:
                mse = torch.nn.functional.mse_loss(image.detach(), gt_image)
                value = l1_ssim_loss(image, image, gt_image, lambda_dssim)
            value.backward()
            optimizer.step()
            record[0, i], record[1, i] = value.detach(), mse.detach()
    host = record[:, :iters].cpu()   # the loop's one host read
    return param.detach(), host[0], host[1]
