"""Drop-in ``diff_gaussian_rasterization`` for WildGaussians on AMD MI355X (gfx950).

Public surface = what ``wildgaussians/method.py:26,1529-1631`` imports and calls, i.e. the surface of the reference's
``submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py``:

* ``GaussianRasterizationSettings`` -- 15-field NamedTuple, same field names and order (reference :175-190)
* ``GaussianRasterizer(raster_settings)`` -- ``nn.Module``; ``forward(means3D, means2D, opacities, shs=None,
  colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None) -> (color, radii, accumulation)`` and
  ``markVisible(positions)`` (reference :192-241)
* ``rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
  raster_settings)`` (reference :21-42)

Semantics kept from the reference: exactly-one-of validation raising ``Exception``; "not provided" inputs are the
zero-sized ``torch.Tensor([])`` sentinel; gradients come back for (means3D, means2D, sh, colors_precomp, opacities,
scales, rotations, cov3Ds_precomp); ``means2D`` is a zero [P,3] carrier whose gradient holds (d/dx_ndc, d/dy_ndc,
sum|.|) (reference backward.cu:590-595, read at method.py:1471-1476); ``radii`` and ``accumulation`` are
non-differentiable; ``debug=True`` dumps the CPU copy of the arguments to snapshot_{fw,bw}.dump when the native call
raises.  The native side is ``_C`` -> ``libwg_rasterizer.so`` (hand-written HIP); there is no CPU/PyTorch fallback.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _C
from . import contributions as _contrib
from .contributions import ContributionStats, collect_contributions   # per-Gaussian contribution statistics (wg_render_contributions)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians"]
call_options = _C.call_options   # `with call_options(deterministic_backward=1): ...` (thread-local, scoped; see _C.py)
colour_gradients_only = _C.colour_gradients_only   # `with colour_gradients_only(True): ...`: the colour-only backward pass as the thread's default
                                                   # (`"fixed_order"` in place of True: without float atomics, bit-identical run to run)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    kernel_size: float
    subpixel_offset: torch.Tensor
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    return_accumulation: bool


def _absent() -> torch.Tensor:
    return torch.Tensor([])


def _call_native(fn, args, debug: bool, dump_path: str, what: str):
    """Run a native entry point; in debug mode keep a CPU copy of the inputs and dump it if the call raises."""
    if not debug:
        return fn(*args)
    saved = tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)
    try:
        return fn(*args)
    except Exception:
        torch.save(saved, dump_path)
        print(f"\nAn error occured in {what}. Writing {dump_path} for debugging.\n")
        raise


def _accumulation_from_image_state(img_buffer: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """accumulation = 1 - final_T (reference __init__.py:101-113).  The forward kernels write it themselves, as the second array of
    the image-state buffer (wg_rasterizer.h): a view, no elementwise kernel per call.  The memory belongs to this call's scratch
    (kept alive by the view); calls that share an image state through the binding's geometry reuse share the values too."""
    align = _C.IMAGE_STATE_ALIGNMENT
    start = (-img_buffer.data_ptr()) % align + _C.accumulation_offset(height, width)
    return img_buffer[start:start + 4 * height * width].view(torch.float32).view(height, width)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                sh_mul=None, sh_offset=None, sh_pre_clamp_max=None, sh_post_clamp_max=None, binning_capacity=None, colors_precomp2=None,
                filter_3D=None, sh_second=False, sh_mul2=None, sh_offset2=None, sh_pre_clamp_max2=None, sh_post_clamp_max2=None, call_options=None,
                colour_gradients_only=None, grad_mode=True, contributions=None, distortion_grad=False, return_distortion=None, depth_grad=False,
                return_depth=None):
        rs = raster_settings
        native_args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                       rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset,
                       rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
        # Everything below is beyond the reference (opt-in by keyword, see GaussianRasterizer.forward) and goes to the native module as the
        # optional blocks of ONE call (include/wg_rasterizer.h: wg_forward_args).
        # per-call options: resolved ONCE here (keyword > the calling thread's defaults) and carried to the backward call on ctx
        ctx.call_options = _C.resolve_call_options(call_options)
        extra = dict(options=ctx.call_options)
        # nothing takes a gradient (grad mode was off at the call -- it always is in here, so the caller passes it --, or no input requires
        # one): no backward call will follow, the frame leaves nothing for one (wg_forward_args::forward_only)
        extra["forward_only"] = not (grad_mode and any(ctx.needs_input_grad))
        # the colour-only backward pass (wg_backward_args::colour_gradients_only): resolved ONCE here too (keyword > the calling thread's default);
        # what it cannot serve is refused now, not in the middle of a backward pass
        ctx.colour_only = _C.resolve_colour_gradients_only(colour_gradients_only)
        toned = any(v is not None for v in (sh_mul, sh_offset, sh_pre_clamp_max, sh_post_clamp_max))
        if ctx.colour_only and _C.colour_only_refused(sh.numel() != 0, toned, colors_precomp2 is not None, filter_3D is not None, bool(sh_second),
                                                      ctx.call_options):
            raise Exception(_C.COLOUR_ONLY_MSG)
        # per-Gaussian affine + clamps on the SH coefficients in-kernel (wg_sh_tone)
        ctx.sh_tone = None
        if sh_mul is not None or sh_offset is not None or sh_pre_clamp_max is not None or sh_post_clamp_max is not None:
            if sh.numel() == 0:
                raise Exception("sh_mul / sh_offset / sh_*_clamp_max act on SH coefficients: provide shs, not colors_precomp")
            ctx.sh_tone = (None if sh_mul is None else sh_mul.detach(), None if sh_offset is None else sh_offset.detach(),
                           sh_pre_clamp_max, sh_post_clamp_max)
            extra["sh_tone"] = ctx.sh_tone
        # the depth pass over the finished frame (wg_render_depth): refused now, before anything is rendered, where it cannot be served
        if return_depth is not None:
            _C.check_depth_source(return_depth, means3D.shape[0])
            # depth_grad: the frame's backward call adds the depth loss's gradient into its gradient record (wg_depth_grad) -- refused now where
            # there is no such record, not in the middle of a backward pass
            if depth_grad and _C.depth_grad_refused(ctx.colour_only, ctx.call_options, binning_capacity is not None):
                raise Exception(_C.DEPTH_GRAD_MSG)
            if binning_capacity is not None:
                raise Exception(_C.DEPTH_CAPACITY_MSG)
        elif depth_grad:
            raise Exception("depth_grad=True is the gradient of the depth output: pass return_depth too")
        # the distortion pass over the finished frame (wg_render_distortion) and its gradient (wg_distortion_grad): refused like the depth pass's
        if return_distortion is not None:
            _C.check_distortion_source(return_distortion, means3D.shape[0])
            if distortion_grad and _C.distortion_grad_refused(ctx.colour_only, ctx.call_options, binning_capacity is not None):
                raise Exception(_C.DISTORTION_GRAD_MSG)
            if binning_capacity is not None:
                raise Exception(_C.DISTORTION_CAPACITY_MSG)
        elif distortion_grad:
            raise Exception("distortion_grad=True is the gradient of the distortion output: pass return_distortion too")
        # the contribution pass over the finished frame (wg_render_contributions): (stats, mask) or None; refused now, before anything is rendered
        contrib_mask = None
        if contributions is not None:
            _contrib.check_stats(contributions[0], means3D.shape[0], means3D.device)
            contrib_mask = _contrib.check_mask(contributions[1], rs.image_height, rs.image_width, means3D.device)
            if binning_capacity is not None:
                raise Exception(_C.CONTRIB_CAPACITY_MSG)
        if binning_capacity is not None:   # no host rendezvous (wg_forward_args::binning_capacity), capturable in a hipGraph
            extra["binning_capacity"] = int(binning_capacity)
        # a second set of precomputed colours composited in the same walk (wg_second_image)
        ctx.dual = colors_precomp2 is not None
        # opacities / scales / rotations are the RAW parameters, get_gaussians() runs in-kernel (wg_raw_gaussians)
        ctx.raw = filter_3D is not None
        if ctx.raw and (ctx.dual or binning_capacity is not None):
            raise Exception("filter_3D (raw-parameter mode) cannot be combined with colors_precomp2 / binning_capacity")
        if ctx.raw:
            extra["filter_3D"] = filter_3D
        # both colour sets from the same SH block, each through its own tone (wg_forward_args::sh_second + tone2)
        ctx.sh_second = None
        if sh_second:
            if sh.numel() == 0 or ctx.dual or binning_capacity is not None:
                raise Exception("sh_second renders a second tone of the SH coefficients: provide shs, and neither colors_precomp2 nor binning_capacity")
            ctx.sh_second = (None if sh_mul2 is None else sh_mul2.detach(), None if sh_offset2 is None else sh_offset2.detach(),
                             sh_pre_clamp_max2, sh_post_clamp_max2)
            extra["sh_second"] = ctx.sh_second
        elif ctx.dual:
            if ctx.sh_tone is not None or binning_capacity is not None:
                raise Exception("colors_precomp2 cannot be combined with sh_mul / sh_offset / binning_capacity")
            extra["colors2"] = colors_precomp2
        res = _call_native(lambda *a: _C.rasterize_gaussians(*a, **extra), native_args, rs.debug, "snapshot_fw.dump", "forward")
        num_rendered, color, radii, geom_buf, binning_buf, img_buf = res[:6]
        color2 = res[6] if len(res) > 6 else None

        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        # radii and accumulation take no gradient (reference backward signature (ctx, grad_out_color, _, _), :117): do not let
        # autograd materialise P- and H*W-sized zero tensors for them on every backward pass
        ctx.set_materialize_grads(False)
        ctx.distortion = return_distortion is not None
        ctx.distortion_grad = ctx.distortion and bool(distortion_grad)
        ctx.distortion_source = None
        distortion = moments = None
        if ctx.distortion:
            # one more walk over the frame just finished, reading its buffers only: the blend weights' centred moments per pixel and A Q' - D'^2 of
            # them.  With distortion_grad the moments are kept for the frame's backward call; without it none are written
            source = return_distortion.detach() if isinstance(return_distortion, torch.Tensor) else return_distortion
            distortion = _call_native(lambda *a: _C.render_distortion(*a, options=ctx.call_options, moments=ctx.distortion_grad, debug=rs.debug),
                                      (geom_buf, binning_buf, img_buf, num_rendered, means3D.shape[0], rs.image_height, rs.image_width, source,
                                       means3D.detach(), rs.campos, rs.subpixel_offset), rs.debug, "snapshot_distortion.dump", "the distortion pass")
            if ctx.distortion_grad:
                distortion, moments = distortion
                ctx.distortion_source = source
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom_buf, binning_buf, img_buf,
                              *((filter_3D, opacities) if ctx.raw else ()), *((moments,) if ctx.distortion_grad else ()))

        accumulation = None
        if rs.return_accumulation:
            if means3D.shape[0] == 0:
                accumulation = torch.zeros((rs.image_height, rs.image_width), dtype=torch.float32, device=color.device)
            else:
                accumulation = _accumulation_from_image_state(img_buf, rs.image_height, rs.image_width)
        out = (color, radii, accumulation, color2) if ctx.dual or ctx.sh_second is not None else (color, radii, accumulation)
        ctx.depth = return_depth is not None
        ctx.depth_grad = ctx.depth and bool(depth_grad)
        ctx.depth_source = None
        nondiff = []
        if ctx.depth:
            # one more walk over the frame just finished, reading its buffers only (whichever call served it: a full one or, with geometry
            # reuse, a recolouring): the image stays differentiable as before, depth takes no gradient
            depth = _call_native(lambda *a: _C.render_depth(*a, options=ctx.call_options, debug=rs.debug),
                                 (geom_buf, binning_buf, img_buf, num_rendered, means3D.shape[0], rs.image_height, rs.image_width,
                                  return_depth.detach() if isinstance(return_depth, torch.Tensor) else return_depth, means3D.detach(), rs.campos,
                                  rs.subpixel_offset), rs.debug, "snapshot_depth.dump", "the depth pass")
            if ctx.depth_grad:   # the scalars go to the backward call as the forward pass read them ("distance": the call's means3D and campos)
                ctx.depth_source = return_depth.detach() if isinstance(return_depth, torch.Tensor) else return_depth
            else:
                nondiff.append(depth)
            out += (depth,)
        if ctx.distortion:   # the call's LAST output, behind depth
            if not ctx.distortion_grad:
                nondiff.append(distortion)
            out += (distortion,)
        if nondiff:   # (one call: a second would replace the first's list)
            ctx.mark_non_differentiable(*nondiff)
        if contributions is not None:
            # and one more that combines what each Gaussian contributed to it into the caller's arrays; the frame is only read, the output
            # tuple is what it was, nothing here takes a gradient
            stats = contributions[0]
            _call_native(lambda *a: _C.render_contributions(*a, options=ctx.call_options, accumulate=True, debug=rs.debug),
                         (geom_buf, binning_buf, img_buf, num_rendered, means3D.shape[0], rs.image_height, rs.image_width, stats.max_weight,
                          stats.hits, stats.weight_sum_q32, contrib_mask, rs.subpixel_offset), rs.debug, "snapshot_contrib.dump",
                         "the contribution pass")
            stats.views += 1
        return out

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, _grad_accumulation, grad_out_color2=None, *more):
        # the cotangents behind the reference's three, in the outputs' order: the second image's, depth's, the distortion's -- each only where the
        # forward call returned the output (the fourth is whichever of them comes first)
        more = [grad_out_color2] + list(more)
        grad_out_color2 = more.pop(0) if (ctx.sh_second is not None or ctx.dual) and more else None
        grad_depth = more.pop(0) if ctx.depth and more else None
        grad_dist = more.pop(0) if ctx.distortion and more else None
        if not ctx.depth_grad:   # (depth was marked non-differentiable: its cotangent is always None)
            grad_depth = None
        if not ctx.distortion_grad:
            grad_dist = None
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom_buf, binning_buf, img_buf = ctx.saved_tensors[:10]
        zeros = lambda: torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        if grad_out_color is None:  # the image itself took no gradient (only radii / accumulation were used downstream)
            grad_out_color = zeros()
        native_args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                       rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.subpixel_offset, grad_out_color, sh,
                       rs.sh_degree, rs.campos, geom_buf, ctx.num_rendered, binning_buf, img_buf, rs.debug)
        extra = dict(options=ctx.call_options, colour_gradients_only=ctx.colour_only)   # the frame's forward call's
        if ctx.colour_only:   # dL_dcolors and nothing else: the geometry inputs' .grad stay as they were
            g_colors = _call_native(lambda *a: _C.rasterize_gaussians_backward(*a, **extra), native_args, rs.debug, "snapshot_bw.dump", "backward")[1]
            return (None, None, None, g_colors) + (None,) * 25
        # dL_dcolors / dL_dcov3D are intermediates of a plain SH + scales/rotations call: wanted only where the input takes a gradient (what is not
        # wanted comes back as None, neither allocated nor stored)
        extra["want"] = (ctx.needs_input_grad[3], ctx.needs_input_grad[7])
        if ctx.sh_tone is not None:
            extra["sh_tone"] = ctx.sh_tone
        if ctx.raw:
            extra["raw"] = tuple(ctx.saved_tensors[10:12])
        if ctx.sh_second is not None or ctx.dual:
            extra["dL_dout_color2"] = zeros() if grad_out_color2 is None else grad_out_color2   # (None: the second image took no gradient)
        if ctx.sh_second is not None:
            extra["sh_second"] = ctx.sh_second
        if grad_depth is not None:   # a loss on depth: one more walk adds its gradient into the record (None: today's call, no walk)
            extra["depth"] = (grad_depth, ctx.depth_source)
        if grad_dist is not None:    # a loss on the distortion: likewise, with the moments its forward pass left
            extra["distortion"] = (grad_dist, ctx.saved_tensors[-1], ctx.distortion_source)
        res = _call_native(lambda *a: _C.rasterize_gaussians_backward(*a, **extra), native_args, rs.debug, "snapshot_bw.dump", "backward")
        (g_means2D, g_colors, g_opacities, g_means3D, g_cov3Ds, g_sh, g_scales, g_rotations) = res[:8]
        g_mul = g_offset = g_colors2 = g_mul2 = g_offset2 = None
        shaped = lambda g, like: None if (g is None or like is None) else g.view(like.shape)
        if ctx.sh_second is not None:
            g_mul, g_offset, g_mul2, g_offset2 = res[8:12]
            if ctx.sh_tone is not None:
                g_mul, g_offset = shaped(g_mul, ctx.sh_tone[0]), shaped(g_offset, ctx.sh_tone[1])
            g_mul2, g_offset2 = shaped(g_mul2, ctx.sh_second[0]), shaped(g_offset2, ctx.sh_second[1])
        elif ctx.dual:
            g_colors2 = res[8]
        elif ctx.sh_tone is not None:
            g_mul, g_offset = shaped(res[8], ctx.sh_tone[0]), shaped(res[9], ctx.sh_tone[1])
        # the scalars' gradient, where return_depth was a tensor that takes one (its place among forward()'s inputs: the last)
        g_values = None
        if grad_depth is not None and isinstance(ctx.depth_source, torch.Tensor) and ctx.needs_input_grad[28]:
            g_values = res[-1].view(ctx.depth_source.shape)
        # ... and the distortion's: in front of depth's in the native result where both blocks went
        g_values_t = None
        if grad_dist is not None and isinstance(ctx.distortion_source, torch.Tensor) and ctx.needs_input_grad[26]:
            g_values_t = res[-2 if grad_depth is not None else -1].view(ctx.distortion_source.shape)
        # order of forward()'s inputs; None for raster_settings, the clamp constants and the options
        return (g_means3D, g_means2D, g_sh, g_colors, g_opacities, g_scales, g_rotations, g_cov3Ds, None, g_mul, g_offset, None, None, None, g_colors2, None,
                None, g_mul2, g_offset2, None, None, None, None, None, None, None, g_values_t, None, g_values)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                        sh_mul=None, sh_offset=None, sh_pre_clamp_max=None, sh_post_clamp_max=None, binning_capacity=None, colors_precomp2=None,
                        filter_3D=None, sh_second=False, sh_mul2=None, sh_offset2=None, sh_pre_clamp_max2=None, sh_post_clamp_max2=None, call_options=None,
                        *, colour_gradients_only=None, return_depth=None, depth_grad=False, contributions=None, contribution_mask=None,
                        return_distortion=None, distortion_grad=False):
    _C._colour_mode(colour_gradients_only)   # (an unknown string: ValueError, before anything touches the device)
    if isinstance(return_distortion, str):
        _C.check_distortion_source(return_distortion)   # (likewise)
    # contributions=: the keyword, else what an open `with collect_contributions(stats, mask)` block of this thread still holds -- its FIRST
    # forward call takes it (handed back if that call raises)
    taken = False
    if contributions is None:
        if contribution_mask is not None:
            raise Exception("contribution_mask masks the contribution pass: pass contributions too")
        contributions, contribution_mask = _contrib.take_pending()
        taken = contributions is not None
    try:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                         raster_settings, sh_mul, sh_offset, sh_pre_clamp_max, sh_post_clamp_max, binning_capacity, colors_precomp2,
                                         filter_3D, sh_second, sh_mul2, sh_offset2, sh_pre_clamp_max2, sh_post_clamp_max2, call_options,
                                         colour_gradients_only, torch.is_grad_enabled(),
                                         None if contributions is None else (contributions, contribution_mask), bool(distortion_grad), return_distortion,
                                         bool(depth_grad), return_depth)
    except BaseException:
        if taken:
            _contrib.restore_pending(contributions, contribution_mask)
        raise


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Boolean mask of points that pass the near-plane test of the preprocess stage (view-space z > 0.2)."""
        rs = self.raster_settings
        with torch.no_grad():
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def project_radii(self, means3D, scales: Optional[torch.Tensor] = None, rotations: Optional[torch.Tensor] = None,
                      cov3D_precomp: Optional[torch.Tensor] = None, *, filter_3D: Optional[torch.Tensor] = None,
                      opacities: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The projection-only pass (beyond the reference): `radii` (int32 [P]) of the frame `forward` would render from these geometry inputs
        through this rasterizer's camera -- the same bits, so `radii > 0` is the frame's visible set -- WITHOUT rendering it: one launch that
        reads the geometry and writes 4 bytes per Gaussian; no colours, no binning, no scratch buffers, no host synchronisation.  Camera, image
        size, `kernel_size` and `scale_modifier` come from `raster_settings`, as in `forward`.  For whatever needs a frame's visible set before
        it has colours (`wg_fused_gaussians.VisibleRows.from_camera`: the appearance MLP over visible rows in front of ONE two-tone call).
        `markVisible` is not this: it is the near-plane test alone and keeps everything in front of the camera, on screen or not.

        `filter_3D=`: `scales` / `rotations` are the caller's RAW parameters, as in `forward(filter_3D=)`.  `opacities=` is accepted so that
        the call can carry `forward`'s geometry arguments, and is not read: no radius depends on an opacity, raw or activated.
        float32 tensors on one HIP device; runs under `torch.no_grad()`."""
        has_scale_rot = scales is not None or rotations is not None
        complete_scale_rot = scales is not None and rotations is not None
        if (cov3D_precomp is None and not complete_scale_rot) or (cov3D_precomp is not None and has_scale_rot):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        rs = self.raster_settings
        with torch.no_grad():
            return _C.project_radii(means3D, scales, rotations, cov3D_precomp, filter_3D, rs.scale_modifier, rs.viewmatrix, rs.projmatrix,
                                    rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.image_height, rs.image_width)

    def forward(self, means3D, means2D, opacities, shs: Optional[torch.Tensor] = None,
                colors_precomp: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                rotations: Optional[torch.Tensor] = None, cov3D_precomp: Optional[torch.Tensor] = None, *,
                sh_mul: Optional[torch.Tensor] = None, sh_offset: Optional[torch.Tensor] = None,
                sh_pre_clamp_max: Optional[float] = None, sh_post_clamp_max: Optional[float] = None,
                binning_capacity: Optional[int] = None, colors_precomp2: Optional[torch.Tensor] = None,
                filter_3D: Optional[torch.Tensor] = None, sh_second: bool = False, sh_mul2: Optional[torch.Tensor] = None,
                sh_offset2: Optional[torch.Tensor] = None, sh_pre_clamp_max2: Optional[float] = None,
                sh_post_clamp_max2: Optional[float] = None, exact_compositing: Optional[bool] = None,
                deterministic_backward: Optional[bool] = None, grad_record: Optional[bool] = None,
                colour_gradients_only=None, return_depth=None, depth_grad: bool = False, contributions=None, contribution_mask=None,
                return_distortion=None, distortion_grad: bool = False):
        """`return_distortion=` (keyword-only, beyond the reference): `"distance"` or a float32 [P] device tensor of per-Gaussian scalars v, the two
        sources of `return_depth`.  The call then returns what it returns otherwise PLUS, as its LAST output (behind `depth` when both are asked
        for), `distortion` ([H, W] float32): the Mip-NeRF 360 / 2DGS distortion term of the frame just rendered,
        sum_{j<i} w_i w_j (v_i - v_j)^2 with w = alpha * T over the (pixel, Gaussian) pairs the frame blended -- the frame's own decisions, no
        background term, no normalisation, 0 for a pixel without a contributor.  One more walk over the finished frame's lists
        (wg_render_distortion) sums the weights' moments CENTRED on each pixel's first blended v and forms A Q' - D'^2: the term is invariant
        under a shift of v, and the centred sums do not cancel where a `colors_precomp = (1, v, v^2)` render's A Q - D^2 does in float32 (thin
        surfaces far from the camera).  Not clamped: a last-bit negative value can come out.  Works under `torch.no_grad()`, with every colour
        source, on a frame served by geometry reuse, beside `return_depth` / `depth_grad` and `contributions=`; refused with
        `binning_capacity`; an unknown string raises ValueError before anything touches the device.  None (the default): nothing new runs.
        `distortion_grad=True` (with `return_distortion=`): `distortion` is DIFFERENTIABLE -- with respect to the call's geometry inputs (with
        `filter_3D=` the RAW parameters), to a `return_distortion` tensor that requires grad, and in `"distance"` mode to `means3D` through
        v = |means3D - campos| as well.  The forward pass then keeps four [H, W] planes of moments, and a loss on the distortion costs ONE more
        per-tile walk in the frame's backward call, adding into the gradient record like `depth_grad`'s (wg_distortion_grad), behind it when both
        are present; `means2D.grad[:, 2]` accumulates |q_dist| beside |q_image|.  A backward pass in which the distortion took no gradient
        launches no walk.  Refused at forward time with `colour_gradients_only`, `deterministic_backward=1`, `grad_record=0` and
        `binning_capacity`, and without `return_distortion`.  False (the default): the output takes no gradient and no moments are kept.

        `contributions=stats` (keyword-only, beyond the reference): a `ContributionStats(P, device)`.  After the frame is finished, one more
        walk over its lists combines into `stats`, per Gaussian and over the (pixel, Gaussian) pairs this call blended, the largest blend
        weight w = alpha * T (`max_weight`), the number of pairs (`hits`) and the sum of floor(w * 2^32) (`weight_sum_q32`), and
        `stats.views` goes up by one (wg_render_contributions).  Integer atomics only: two sweeps give the same bits.  The published
        pruning criteria are functions of these three (`stats.keep_mask(...)`; wg_integration.prune_by_contribution).
        `contribution_mask=`: bool or float32, [H, W] or [1, H, W]; a pixel whose entry is 0 / False takes no part (the training mask, a
        thresholded uncertainty).  The output tuple is unchanged and nothing takes a gradient.  Works under `torch.no_grad()`, with every
        colour source, on a frame served by geometry reuse and beside `return_depth`; refused with `binning_capacity`; a wrong type, shape,
        dtype or device raises before anything is rendered.  None = what an open `with collect_contributions(stats, mask):` block of the
        calling thread holds, which feeds the FIRST forward call of the block only (a caller's render makes two or three calls over the same
        geometry); no block: nothing new runs.

        `depth_grad=True` (keyword-only, beyond the reference; with `return_depth=`): `depth` is DIFFERENTIABLE -- with respect to the call's
        geometry inputs (`means3D`, `means2D` as the carrier of the screen-space gradient, `opacities`, `scales` / `rotations` or `cov3D_precomp`;
        with `filter_3D=` the RAW parameters), to a `return_depth` tensor that requires grad, and in `"distance"` mode to `means3D` through
        v = |means3D - campos| as well (`campos` is a settings field and takes none).  A loss on depth then costs ONE more per-tile walk in the
        frame's backward call, which adds its sums into the gradient record the image walk fills before the per-Gaussian kernel reads it
        (wg_depth_grad) -- in place of a second three-channel call with the distances as colours and its whole backward pass.  The gradients are
        those two calls would give added up; `means2D.grad[:, 2]`, the densification statistic, accumulates |q_depth| beside |q_image| as they
        would.  A backward pass in which depth took no gradient is the call without the keyword: no walk is launched.  A backward pass with only
        a depth cotangent runs the image walk on a zero image cotangent.  Refused at forward time with `colour_gradients_only`,
        `deterministic_backward=1`, `grad_record=0` and `binning_capacity` (it needs the atomic gradient record), and without `return_depth`.
        False (the default): depth takes no gradient, as before.

        `return_depth=` (keyword-only, beyond the reference): `"distance"` or a float32 [P] device tensor of per-Gaussian scalars.  The call
        then returns what it returns otherwise PLUS, as its LAST output, `depth` ([H, W] float32): the scalar composited over the frame just
        rendered like a colour channel -- sum over the blended (pixel, Gaussian) pairs of v * alpha * T, with the frame's own decisions, no
        background term and no division by the accumulation.  `"distance"` is v = |means3D - campos|: the image WildGaussians' depth render
        (method.py:1621-1631: `torch.norm(means3D - camera_center[None], dim=-1)` repeated to three channels through a second rasterizer call
        over a zero background) keeps one channel of -- here one more single-channel walk over the finished frame's lists instead of a second
        projection, binning, sort and three-channel walk (wg_render_depth).  A tensor gives any scalar attribute (view-space z, a label
        weight, ...) the same treatment, with the bits of one channel of `colors_precomp=v[:, None].repeat(1, 3)`.  Depth takes no gradient
        (unless `depth_grad=True`, above); the colour outputs stay differentiable exactly as without it.  Works under `torch.no_grad()`, with every colour source of the call and on a
        frame served by geometry reuse; refused with `binning_capacity`.  None (the default): outputs and gradients are what they were.

        `colour_gradients_only=True` (keyword-only, beyond the reference; with `colors_precomp`): the frame's backward pass computes the
        gradient of `colors_precomp` ALONE -- one walk that sums the forward pass's blend weights, no geometry gradients, no per-Gaussian pass;
        every other input's gradient is None (its `.grad` is left as it was).  For steps whose geometry is frozen and whose appearance alone is
        optimised (WildGaussians.optimize_embedding, method.py:1755-1830).  None = the calling thread's default
        (`with colour_gradients_only(True): ...`).  Refused with `shs`, `sh_mul` / `sh_offset` / clamps, `colors_precomp2`, `filter_3D`,
        `sh_second` and `deterministic_backward=1`.
        `colour_gradients_only="fixed_order"`: the same gradient, the same calls served and refused, WITHOUT float atomics -- every (tile,
        Gaussian) term goes to a slot of the library's leased scratch (17 bytes per instance) and a second kernel adds each Gaussian's terms
        in an order fixed by the frame, so two runs give the same bits (for reproducible test-time embedding fits).  Any other string raises
        ValueError.  Not capturable in a hipGraph (the scratch is leased per call).

        `exact_compositing=` / `deterministic_backward=` / `grad_record=` (keyword-only, beyond the reference): the three switches that affect
        results, PER CALL (wg_call_options, include/wg_rasterizer.h); None = the calling thread's default (`_C.call_options(...)` sets it for a
        `with` block -- for callers that cannot pass keywords); the frame's backward pass runs with its forward call's values.

        `sh_second=True` (keyword-only, beyond the reference; with `shs`): a SECOND image from the same SH coefficients through a tone
        of its own (`sh_mul2` / `sh_offset2` / `sh_*_clamp_max2`, each optional), composited in the SAME call as the first -- WildGaussians'
        step (method.py:1573-1611) renders the raw and the toned colours of one SH block: `rast(shs=f, sh_mul=mul, sh_offset=offset / C0,
        sh_pre_clamp_max=1, sh_post_clamp_max=1, sh_second=True, sh_pre_clamp_max2=1)` returns `(toned, radii, accumulation, raw)` from one
        projection, one binning, one forward and one backward walk.  Gradients flow to `shs` (both images' losses), and to each tone's
        `mul` / `offset`.  Composes with `filter_3D`.

        `filter_3D=` (keyword-only, beyond the reference): `opacities`, `scales`, `rotations` are then the caller's RAW
        parameters (logit, log-scale, unnormalised quaternion) and `get_gaussians()` (method.py:1060-1086: normalise, exp, sigmoid, 3-D
        filter with this [P,1] tensor) runs inside the preprocess kernels, forward and backward: the gradients returned for those three
        inputs are the raw parameters'.  Composes with `shs` + `sh_mul` / `sh_offset` (the whole step before the operator in-kernel).

        `colors_precomp2=` (keyword-only, beyond the reference; with `colors_precomp`): a second [P,3] colour set composited in the SAME
        call -- one projection, one binning, one forward and one backward walk for both (WildGaussians' raw and toned colours,
        method.py:1573-1611).  Returns `(color, radii, accumulation, color2)`; gradients flow to both colour
        tensors, the geometry gradients are those of both images' losses together.

        `binning_capacity=` (keyword-only, beyond the reference): the forward pass without any host rendezvous
        (wg_forward_args::binning_capacity: the caller supplies the number of (tile, Gaussian) instances the binning buffer holds), for steps
        captured in a hipGraph; a frame that does not fit comes back as NaN, `_C.forward_status` tells.  Otherwise:

        The reference's signature (diff_gaussian_rasterization/__init__.py:208-241) plus four keyword-only opt-ins (SURVEY.md 8f
        N3): with `shs`, the kernels evaluate `min(min(shs, sh_pre_clamp_max) * sh_mul[:, None, :] + [k == 0] * sh_offset[:, None, :],
        sh_post_clamp_max)` instead of `shs` -- WildGaussians' appearance toning (method.py:890-900, 1590-1595: pass the clamped
        features' raw tensor, `mul`, `offset / C0`, and 1.0 for both clamps) without the P x 48 intermediate tensors -- and return
        gradients for `shs` (raw), `sh_mul` and `sh_offset` ([P, 3] each)."""
        _C._colour_mode(colour_gradients_only)   # (an unknown string: ValueError, before anything touches the device)
        if isinstance(return_distortion, str):
            _C.check_distortion_source(return_distortion)   # (likewise)
        if (shs is None) == (colors_precomp is None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if colors_precomp2 is not None and colors_precomp is None:
            raise Exception('colors_precomp2 is a second set of precomputed colours: provide colors_precomp too')
        has_scale_rot = scales is not None or rotations is not None
        complete_scale_rot = scales is not None and rotations is not None
        if (cov3D_precomp is None and not complete_scale_rot) or (cov3D_precomp is not None and has_scale_rot):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        return rasterize_gaussians(
            means3D, means2D,
            _absent() if shs is None else shs,
            _absent() if colors_precomp is None else colors_precomp,
            opacities,
            _absent() if scales is None else scales,
            _absent() if rotations is None else rotations,
            _absent() if cov3D_precomp is None else cov3D_precomp,
            self.raster_settings, sh_mul, sh_offset, sh_pre_clamp_max, sh_post_clamp_max, binning_capacity, colors_precomp2, filter_3D,
            sh_second, sh_mul2, sh_offset2, sh_pre_clamp_max2, sh_post_clamp_max2,
            None if exact_compositing is None and deterministic_backward is None and grad_record is None else
            dict(exact_compositing=exact_compositing, deterministic_backward=deterministic_backward, grad_record=grad_record),
            colour_gradients_only=colour_gradients_only, return_depth=return_depth, depth_grad=depth_grad,
            contributions=contributions, contribution_mask=contribution_mask, return_distortion=return_distortion, distortion_grad=distortion_grad)
