"""Run-time opt-ins for the reference's caller, WITHOUT editing its source.

    import wildgaussians.method as method          # the reference's module, unchanged on disk
    import wg_integration
    undo = wg_integration.apply_optins(method)     # before or after the model is built
    ...
    undo()                                          # puts the original attributes back

Only pieces that are module- or class-level names can be swapped this way; what is written inline in `_render_internal` /
`train_iteration` (SH evaluation and appearance toning in the operator, the fused L1 + DSSIM loss, `subpixel_offset=None`) still
needs the few-line edits INTEGRATION.md lists.  What IS swapped, each with the results its tests pin:

  ssim                  `method.ssim` (method.py:644-673, called at :1949)           -> wg_fused_ssim.ssim (same signature)
  adam                  `GaussianModel._setup_optimizers` (method.py:1029-1054)      -> the same, then FusedAdam.adopt(self.optimizer);
                        an optimizer that already exists on `model` is adopted at once (pass `model=`)
  densification_stats   `GaussianModel.add_densification_stats` (method.py:1470-1477) -> wg_fused_gaussians.add_densification_stats
  activations           `GaussianModel.get_gaussians` (method.py:1060-1086)          -> wg_fused_gaussians.activate (same dict)
  eval_sh               `method.eval_sh` (method.py:493-548, called at :1564, :1597) -> wg_fused_gaussians.eval_sh; calls it does not cover
                        (degree 4, a channel count other than 3, CPU tensors) go to the original function
  filter_3d             (OFF by default, unlike the switches above: a visibility decision at a screen border or at the near limit can fall
                        the other way than torch's matmul makes it fall, and callers' pinned results must not move unasked)
                        `GaussianModel.compute_3D_filter` (method.py:1140-1190) -> wg_fused_gaussians.compute_3D_filter with one
                        CameraTable per `cameras` object (built at its first call); the buffer is registered as the reference does
  densify               (OFF by default, like filter_3d and for the same reason: a clone / split / prune decision that sits within an ulp of its
                        threshold can fall the other way than torch's `exp` / `sigmoid` make it fall)
                        `GaussianModel.densify_and_prune` (method.py:1420-1468, with _densify_and_clone, _densify_and_split,
                        _densification_postfix, _prune_points) -> wg_fused_gaussians.densify_and_prune: one plan, one host wait, one gather;
                        parameters and buffers are re-registered and `optimizer.state` re-keyed as the reference does (a new nn.Parameter
                        per group, the state moved to it).  `GaussianModel.reset_opacity` (method.py:1249-1278) ->
                        wg_fused_gaussians.reset_opacity.  The split's draw is torch.randn on the device
  visible_adam          (OFF by default: results differ from dense Adam BY DESIGN; only with adam, else ValueError)
                        `_setup_optimizers`, and an optimizer that already exists on `model`, adopt into wg_fused_gaussians.VisibleRowsAdam
                        instead of FusedAdam, and `GaussianModel._render_internal` (the caller's own or edited_module's) is wrapped: a render
                        in training mode with grad mode on hands its `radii` to `self.optimizer.visible(...)`, and the `optimizer.step()` that
                        follows (method.py:2019) updates, in the seven per-Gaussian groups, only the rows with radii > 0 (3D-GS's sparse_adam,
                        gsplat's SelectiveAdam; include/wg_adam_rows.h).  Unlisted Gaussians keep parameter and both moments; a loss term that
                        gives invisible Gaussians a non-zero gradient is ignored for them; the bias correction follows the global step count.
                        The list lasts one step.  Evaluation renders and `optimize_embedding` run in eval mode and leave none behind; in the
                        densification step the caller's `densify_and_prune` replaces the parameters before `step()`, which then skips them
                        (no gradient) and drops the list
  uncertainty_metrics   (OFF by default: results move within float32 rounding, and callers' logged metrics must not move unasked)
                        `method.msssim` (method.py:171-187) and `method.ssim_down` (:126-135), which UncertaintyModel._compute_losses
                        looks up as module globals on every step -> wg_fused_ssim.msssim / ssim_down (forward only); calls they do not
                        cover (CPU tensors, a dtype other than float32, an input that requires grad) go to the original functions
  uncertainty_loss      (OFF by default: results move within float32 rounding, logged metrics move with them, and the dropout mask is drawn
                        by another call than the reference's, so the random stream may differ)
                        `UncertaintyModel._compute_losses` (method.py:363-433) -> wg_fused_uncertainty.compute_losses: everything around the
                        frozen backbone (the three normalise / pad / resize chains, dropout2d + batch norm + the 1x1 convolution + softplus,
                        the full-resolution maps and their six reductions, the cosine similarity, the DINO loss, the backward pass into
                        conv_seg and bn) in HIP kernels, the metrics read with ONE device-to-host copy.  The backbone is still called
                        through the model's own `_get_dino_cached`.  Calls it does not cover (another uncertainty_mode,
                        uncertainty_dino_max_size set, CPU tensors, a batch, a prediction that requires grad, an initialised process
                        group, a head of another form) go to the original method
  uncertainty_backbone  (OFF by default: results move within float32 rounding)
                        `UncertaintyModel._get_dino_cached` (method.py:257-265) -> the same statements, except that a covered backbone call
                        (`dinov2_vits14_reg`'s architecture in float32 on a HIP device, a float32 [B, 3, 14 h, 14 w] input; wg_fused_dino) is
                        served by a wg_fused_dino.DinoFeatures kept on the model object: blocks 0..num_heads - 1 only, attention with an online
                        softmax, no N x N tensor.  The cache keeps the reference's keys, shapes and contents (`.detach().cpu()` stays).  Every
                        uncovered call reaches the original method with the caller's arguments.  Composes with `uncertainty_loss` (which calls
                        the model's `_get_dino_cached`) and with keep_training_frames_on_device(features=True)
  uncertainty_feature_cache  (OFF by default: it changes memory use, 15.2 MB per 1600x1200 frame; only with uncertainty_backbone, else ValueError)
                        a stored entry is ALSO registered under the key the reference looks up, (cache_entry, input shape) -- the same tensor
                        object, no second copy -- so a frame's ground-truth features are computed once instead of at every visit.  No result
                        changes: the fused extractor is bit-reproducible, the cached tensor is the recomputed one
  appearance_mlp        (OFF by default: results move within float32 rounding)
                        `EmbeddingModel.forward` (method.py:890-900) -> wg_fused_gaussians.embedding_forward: `cat`, the three Linear
                        layers, both ReLUs and `* 0.01` as one float32 MFMA kernel forward and one backward that recomputes the hidden
                        activations (nothing of size P x 128 is kept or written); the two toning statements stay torch.  An `aembedding`
                        of shape [E] takes the shared path.  Calls it does not cover (CPU tensors, a dtype other than float32,
                        appearance_model_sh = True, an `mlp` that is not Linear-ReLU-Linear-ReLU-Linear with 128 / 128 / 6) go to the
                        original forward.
                        Over the visible rows only (off unless the caller asks): inside
                            with wg_fused_gaussians.appearance_rows(wg_fused_gaussians.VisibleRows.from_radii(radii)):
                        -- the one-line edit of `_render_internal` around method.py:1592, `radii` being what the raw call at :1574
                        returned -- the swapped forward evaluates the rows with radii > 0 only, forward and
                        backward, and returns zeros at the others, which the toned call of the same geometry never reads.  A list built
                        for another row count raises; no list is ever guessed from an earlier rasterizer call.  The `two_tone`
                        single-call edit has no `radii` before the MLP: it is either the two calls with `geometry_reuse` and the row
                        list, or one call and the dense MLP
  edited_module         (off by default) `GaussianModel._render_internal` -> the one of a module the INTEGRATOR supplies: a copy of the caller with
                        INTEGRATION.md section 5's "two_colour" or "two_tone" edit applied (the documented diff is the deliverable; this package
                        does not rewrite anybody's source -- tests/real_caller/render_edits.py is the test tool that builds such a module in memory)
  embedding_optim       (OFF by default: the geometry parameters' `.grad` stay None instead of being filled and then zeroed)
                        `WildGaussians.optimize_embedding` (method.py:1755-1830: 128 render-and-backward steps per test image whose only
                        parameter is the appearance embedding, reached through `colors_precomp`) runs inside
                        `diff_gaussian_rasterization.colour_gradients_only(True)`: every backward pass is the colour-only one
                        `embedding_optim="fixed_order"`: inside `colour_gradients_only("fixed_order")` instead -- no float atomics, so two fits of
                        one checkpoint and image end at the same embedding, bit for bit (docs/OPTIONS.md)
                        Not with `edited_module` (ValueError): its render passes a second colour set or SH colours, which that pass refuses
  geometry_reuse        library option "geometry_reuse" = 1 (opt-in since round 4): the toned and depth calls of `_render_internal`
                        (method.py:1573-1631) ride on the raw call's projection and binning.  The caller's training loop qualifies
                        (it writes geometry only between a backward pass and the next forward pass); undo() switches it off again

A switch of its own, on a TRAINER object instead of the module, and off unless called (it changes device memory use):

    undo = wg_integration.keep_training_frames_on_device(trainer)     # after WildGaussians.setup_train
  frames on the device  `trainer.train_images`, `trainer.train_masks` (method.py:1716-1723, fetched at :1917-1918) -> wg_frame_store.FrameList:
                        8-bit frames live on the device as uint8 and every access is one HIP kernel that writes the float32 tensor
                        `.to(device)` would deliver, bit for bit; `uncertainty_model._images_cache` (method.py:262-264) ->
                        wg_frame_store.FeatureCache, whose values stay on the device.  The caller's `.to(device)` lines become no-ops

And one on the EVALUATION module (`wildgaussians.evaluation`, not `method`), off unless called (logged metrics move within rounding):

    undo = wg_integration.fuse_evaluation_metrics(evaluation)         # before the evaluation protocol object is built
  evaluation metrics    `evaluation.compute_metrics` (evaluation.py:331-352) -> wg_fused_metrics.compute_metrics: MSE, MAE and dm_pix's SSIM of
                        every image pair in one HIP kernel and a finishing launch (float32 values and products, float64 filtering, as NumPy
                        computes them), three doubles read back; LPIPS stays the module's own `lpips` / `lpips_vgg`.  Calls it does not cover
                        (anything but two uint8 / float32 NumPy arrays [..., H, W, C] with C <= 4 and H, W >= 11, no HIP device) go to the
                        original function

And one more on the same module, off unless called (logged LPIPS values move within float32 rounding):

    undo = wg_integration.fuse_evaluation_lpips(evaluation)           # any time: `lpips_alex` / `lpips_vgg` look `_lpips` up when called
  evaluation LPIPS      `evaluation._lpips` (evaluation.py:255-291) -> the same result from wg_fused_lpips.LPIPS: both images through the AlexNet
                        or VGG16 trunk as one batch of implicit-GEMM convolutions on float32 MFMA, clip / `* 2 - 1` / scaling layer applied
                        while the first layer loads, one head kernel per tap, float64 pixel sums.  The network is the CALLER's: while
                        `_LPIPS_CACHE` has no entry for `net` the call goes to the original function, which builds (downloads) and caches
                        it; from then on a covered call reads that object's weights.  Calls it does not cover (anything but two float NumPy
                        arrays of one shape [..., H, W, 3], a version other than "0.1", a module that is not the v0.1 alex / vgg model in eval
                        mode and float32, H or W under 31 / 16, no HIP device) go to the original function with the caller's arguments
"""
from __future__ import annotations

import torch


def apply_optins(method_module, model=None, ssim: bool = True, adam: bool = True, densification_stats: bool = True, activations: bool = True,
                 eval_sh: bool = True, geometry_reuse: bool = True, edited_module=None, filter_3d: bool = False, densify: bool = False,
                 visible_adam: bool = False, embedding_optim=False, uncertainty_loss: bool = False, uncertainty_backbone: bool = False,
                 uncertainty_feature_cache: bool = False, appearance_mlp: bool = False, uncertainty_metrics: bool = False):
    """-> a function that restores everything that was replaced.  `model`: an already constructed GaussianModel (e.g.
    `WildGaussians(...).model`) whose existing optimizer should be adopted too.
    edited_module (default None): a module object holding a copy of the caller with INTEGRATION.md section 5's edit of `_render_internal`
    applied (the raw and the toned render in ONE rasterizer call); its `GaussianModel._render_internal` ALSO replaces the caller's, and it is
    handed the swapped `ssim` / `eval_sh`."""
    import wg_fused_gaussians as FG
    import wg_fused_ssim
    if uncertainty_feature_cache and not uncertainty_backbone:
        raise ValueError("uncertainty_feature_cache needs uncertainty_backbone: only the fused extractor is bit-reproducible, so that a cached "
                         "feature map is the one a recomputation would give")
    if visible_adam and not adam:   # before anything is swapped
        raise ValueError("visible_adam needs adam: it is the fused optimizer that takes the row list")
    saved = []

    def swap(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    GM = method_module.GaussianModel
    if ssim:
        swap(method_module, "ssim", wg_fused_ssim.ssim)
    if adam:
        orig_setup = GM._setup_optimizers
        adam_class = FG.VisibleRowsAdam if visible_adam else FG.FusedAdam

        def _setup_optimizers(self):
            orig_setup(self)
            self.optimizer = adam_class.adopt(self.optimizer)
        swap(GM, "_setup_optimizers", _setup_optimizers)
        if model is not None and getattr(model, "optimizer", None) is not None and not isinstance(model.optimizer, adam_class):
            saved.append((model, "optimizer", model.optimizer))
            model.optimizer = adam_class.adopt(model.optimizer)
    if densification_stats:
        def add_densification_stats(self, viewspace_point_tensor, update_filter):
            # the kernel's visibility test is radii > 0: the boolean filter IS that test's result (method.py:1622), as 0 / 1
            gof = self.config.use_gof_abs_gradient
            FG.add_densification_stats(update_filter.to(torch.int32), viewspace_point_tensor.grad, self.xyz_grad, self.denom,
                                       xyz_gradient_accum_abs=self.xyz_gradient_accum_abs if gof else None,
                                       xyz_gradient_accum_abs_max=self.xyz_gradient_accum_abs_max if gof else None)
        swap(GM, "add_densification_stats", add_densification_stats)
    if activations:
        def get_gaussians(self):
            features = self.features_dc
            if self.features_rest is not None:
                features = torch.cat((features, self.features_rest), dim=-1)
            opacities, scales, rotations = FG.activate(self.opacities, self.scales, self.rotations, self.filter_3D)
            return {"xyz": self.xyz, "opacities": opacities, "scales": scales, "rotations": rotations, "features": features}
        swap(GM, "get_gaussians", get_gaussians)

    if eval_sh:
        orig_eval_sh = method_module.eval_sh

        def fused_eval_sh(deg, sh, dirs):
            d = int(deg)
            if (d > 3 or not torch.is_tensor(sh) or not torch.is_tensor(dirs) or sh.dim() < 2 or sh.shape[-2] != 3 or not sh.is_cuda
                    or sh.dtype != torch.float32 or dirs.dtype != torch.float32):
                return orig_eval_sh(deg, sh, dirs)   # the caller's own code, not a fallback of this library
            return FG.eval_sh(d, sh, dirs)
        swap(method_module, "eval_sh", fused_eval_sh)

    if filter_3d:
        tables = {}   # id(cameras) -> CameraTable; the table holds a reference to its cameras object, so the id stays that object's

        def compute_3D_filter(self, cameras):
            xyz = self.xyz
            table = tables.get(id(cameras))
            if table is None or table.cameras is not cameras or table.device != xyz.device:
                table = tables[id(cameras)] = FG.CameraTable(cameras, device=xyz.device)
            filter_3D = FG.compute_3D_filter(xyz, table).to(dtype=self.filter_3D.dtype, device=self.filter_3D.device)
            del self.filter_3D   # as the reference registers its result (method.py:1188-1190)
            self.register_buffer("filter_3D", filter_3D)
        swap(GM, "compute_3D_filter", compute_3D_filter)

    if densify:
        def densify_and_prune(self, max_grad, min_opacity, extent, enable_size_pruning, skyradius=None):
            del skyradius  # unused, as in the reference
            assert self.optimizer is not None, "Not set up for training"
            props = [n for n in self._dynamically_sized_props if getattr(self, n, None) is not None]
            groups = {g["name"]: g for g in self.optimizer.param_groups if g.get("name") in props}
            state = {n: self.optimizer.state.get(g["params"][0], None) for n, g in groups.items()}
            state = {n: st if st is not None and "exp_avg" in st else None for n, st in state.items()}
            res = FG.densify_and_prune({n: g["params"][0] for n, g in groups.items()}, state,
                                       {n: getattr(self, n) for n in props if n not in groups},
                                       max_grad=max_grad, min_opacity=min_opacity, extent=extent, percent_dense=self.config.percent_dense,
                                       enable_size_pruning=enable_size_pruning, use_abs_gradient=bool(self.config.use_gof_abs_gradient))
            for n, g in groups.items():   # _densification_postfix / _prune_points: a new Parameter per group, its state moved to it
                old = g["params"][0]
                new = torch.nn.Parameter(res.tensors[n].requires_grad_(True))
                if state[n] is not None:
                    stored = self.optimizer.state[old]
                    stored["exp_avg"], stored["exp_avg_sq"] = res.adam_state[n]
                    del self.optimizer.state[old]
                    self.optimizer.state[new] = stored
                g["params"][0] = new
                self.register_parameter(n, new)
            for n, t in res.stats.items():
                self.register_buffer(n, t.view(-1, *getattr(self, n).shape[1:]))
            return res.counts
        swap(GM, "densify_and_prune", densify_and_prune)

        def reset_opacity(self):
            assert self.optimizer is not None, "Not set up for training"
            for group in self.optimizer.param_groups:
                if group.get("name") == "opacities":
                    old = group["params"][0]
                    stored = self.optimizer.state.get(old, None)
                    have = stored is not None and "exp_avg" in stored
                    new = FG.reset_opacity(old, self.scales, self.filter_3D, stored["exp_avg"] if have else None,
                                           stored["exp_avg_sq"] if have else None)
                    if stored is not None:
                        del self.optimizer.state[old]
                    group["params"][0] = torch.nn.Parameter(new.requires_grad_(True))
                    self.register_parameter("opacities", group["params"][0])
                    if stored is not None:
                        self.optimizer.state[group["params"][0]] = stored
        swap(GM, "reset_opacity", reset_opacity)

    if uncertainty_metrics:
        orig_msssim, orig_ssim_down = method_module.msssim, method_module.ssim_down

        def covered(*images):
            return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and not t.requires_grad and t.dim() in (3, 4)
                       for t in images)

        def fused_msssim(x, y, max_size=None, min_size=200):
            if not covered(x, y):
                return orig_msssim(x, y, max_size=max_size, min_size=min_size)   # the caller's own code, not a fallback of this library
            return wg_fused_ssim.msssim(x, y, max_size=max_size, min_size=min_size)

        def fused_ssim_down(x, y, max_size=None):
            if not covered(x, y):
                return orig_ssim_down(x, y, max_size=max_size)
            return wg_fused_ssim.ssim_down(x, y, max_size=max_size)
        swap(method_module, "msssim", fused_msssim)
        swap(method_module, "ssim_down", fused_ssim_down)

    if uncertainty_loss:
        import wg_fused_uncertainty
        UM = method_module.UncertaintyModel
        orig_compute_losses = UM._compute_losses

        def _compute_losses(self, gt, prediction, prefix='', _cache_entry=None):
            return wg_fused_uncertainty.compute_losses(self, gt, prediction, prefix, _cache_entry=_cache_entry, original=orig_compute_losses)
        swap(UM, "_compute_losses", _compute_losses)

    if uncertainty_backbone:
        import wg_fused_dino
        UM = method_module.UncertaintyModel
        orig_get_dino_cached = UM._get_dino_cached

        def extractor_for(self, x):
            """The model's DinoFeatures (one per backbone object, kept on the model) when backbone and tensor are the covered case, else None."""
            backbone = getattr(self, "backbone", None)
            ex = self.__dict__.get("_wg_dino_features")
            if ex is None or ex.backbone is not backbone:
                if not wg_fused_dino.DinoFeatures.covers(backbone, x):
                    return None
                ex = self.__dict__["_wg_dino_features"] = wg_fused_dino.DinoFeatures(backbone)
            return ex if ex.input_covered(x) else None

        def _get_dino_cached(self, x, cache_entry=None):
            extractor = extractor_for(self, x)
            if extractor is None:
                return orig_get_dino_cached(self, x, cache_entry)   # the caller's own code, not a fallback of this library
            if cache_entry is None or (cache_entry, x.shape) not in self._images_cache:
                input_shape = x.shape
                with torch.no_grad():
                    x = extractor.features(x)   # the caller's self.backbone.get_intermediate_layers(x, n=[num_heads - 1], reshape=True)[-1]
                if cache_entry is not None:
                    stored = x.detach().cpu()
                    self._images_cache[(cache_entry, x.shape)] = stored
                    if uncertainty_feature_cache:
                        self._images_cache[(cache_entry, input_shape)] = stored   # the key the look-up above asks for; the same object
            else:
                x = self._images_cache[(cache_entry, x.shape)].to(x.device)
            return x
        swap(UM, "_get_dino_cached", _get_dino_cached)

    if appearance_mlp:
        EM = method_module.EmbeddingModel
        orig_embedding_forward = EM.forward

        def embedding_forward(self, gembedding, aembedding, color, viewdir=None):
            return FG.embedding_forward(self, gembedding, aembedding, color, viewdir, original_forward=orig_embedding_forward,
                                        rows=FG.current_appearance_rows())
        swap(EM, "forward", embedding_forward)

    if embedding_optim:
        if isinstance(embedding_optim, str) and embedding_optim != "fixed_order":
            raise ValueError(f"embedding_optim is True, False or 'fixed_order', not {embedding_optim!r}")
        colour_mode = "fixed_order" if isinstance(embedding_optim, str) else True
        if edited_module is not None:   # its _render_internal passes colors_precomp2= / shs= + sh_second=, which the colour-only pass refuses
            raise ValueError("embedding_optim cannot be combined with edited_module: the edited _render_internal makes calls the colour-only "
                             "backward pass refuses (a second colour set, SH colours with tones)")
        WG = method_module.WildGaussians
        orig_optimize_embedding = WG.optimize_embedding

        def optimize_embedding(self, *args, **kwargs):
            from diff_gaussian_rasterization import colour_gradients_only
            with colour_gradients_only(colour_mode):
                return orig_optimize_embedding(self, *args, **kwargs)
        swap(WG, "optimize_embedding", optimize_embedding)

    if edited_module is not None:
        edited = edited_module
        for name in ("ssim", "eval_sh"):   # the edited function looks module-level names up in ITS module: hand it the swapped ones
            swap(edited, name, getattr(method_module, name))   # (undo() puts its own back: the module object is cached in sys.modules)
        swap(GM, "_render_internal", edited.GaussianModel._render_internal)

    if visible_adam:
        inner_render = GM._render_internal   # whatever is in place now: the caller's own, or edited_module's

        def _render_internal(self, *args, **kwargs):
            out = inner_render(self, *args, **kwargs)
            optimizer = getattr(self, "optimizer", None)
            if self.training and torch.is_grad_enabled() and isinstance(optimizer, FG.VisibleRowsAdam):
                optimizer.visible(out["radii"])   # for the step that follows this frame only; compacted on the device when that step runs
            return out
        swap(GM, "_render_internal", _render_internal)

    reuse_before = None
    if geometry_reuse:
        from diff_gaussian_rasterization import _C
        reuse_before = _C.get_option("geometry_reuse")
        _C.set_option("geometry_reuse", 1)

    def undo():
        while saved:
            obj, name, old = saved.pop()
            setattr(obj, name, old)
        if reuse_before is not None:
            from diff_gaussian_rasterization import _C
            _C.set_option("geometry_reuse", reuse_before)
            _C.forget_geometry()
    return undo


def keep_training_frames_on_device(trainer, device=None, max_device_bytes=None, features: bool = True):
    """Keep what `WildGaussians.train_iteration` fetches from the host on every step on the device instead (wg_frame_store): swaps
    `trainer.train_images`, `trainer.train_masks` (when not None) and, with `features`, `trainer.model.uncertainty_model._images_cache` (when
    there is such a model).  -> a function that puts the original lists back, untouched, and a plain dict holding CPU copies of every cached
    feature entry (those added meanwhile included).  The function carries the stand-ins as `.images`, `.masks`, `.features` and their figures
    as `.stats()`.  Off unless called.  device: default the current HIP device.  max_device_bytes: the budget all three share, in the order
    images, masks, features; default half of the device memory that is free now.  What the budget does not admit, and tensors the store
    does not cover, are served from the host as before."""
    from wg_frame_store import Budget, FeatureCache, FrameList
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    budget = Budget(max_device_bytes, device)
    saved = []

    def swap(obj, name, new):
        saved.append((obj, name, getattr(obj, name), new))
        setattr(obj, name, new)
        return new

    images = swap(trainer, "train_images", FrameList(trainer.train_images, device, budget))
    masks = None
    if getattr(trainer, "train_masks", None) is not None:
        masks = swap(trainer, "train_masks", FrameList(trainer.train_masks, device, budget))
    cache, uncertainty_model = None, getattr(getattr(trainer, "model", None), "uncertainty_model", None)
    if features and uncertainty_model is not None and isinstance(getattr(uncertainty_model, "_images_cache", None), dict):
        cache = FeatureCache(device, budget, initial=uncertainty_model._images_cache)
        uncertainty_model._images_cache = cache

    def undo():
        nonlocal cache
        while saved:
            obj, name, old, new = saved.pop()
            new.release()
            setattr(obj, name, old)
        if cache is not None:
            uncertainty_model._images_cache = cache.to_host_dict()
            cache.clear()
            cache = None

    undo.images, undo.masks, undo.features = images, masks, cache
    undo.stats = lambda: {"budget_bytes": budget.total, "used_bytes": budget.used, "images": images.stats(),
                          "masks": masks.stats() if masks is not None else None,
                          "features": undo.features.stats() if undo.features is not None else None}
    return undo


def fuse_evaluation_metrics(evaluation_module):
    """Swap `evaluation_module.compute_metrics` (the reference's wildgaussians/evaluation.py:331-352) for a wrapper over
    wg_fused_metrics.compute_metrics.  -> a function that puts the original back.  Off unless called.

    The wrapper takes the fused path when both arguments are NumPy arrays of dtype uint8 or float32 with the same leading shape
    [..., H, W], at least three dimensions, at most 4 channels after the reference's channel slice (`pred[..., :gt.shape[-1]]`) and
    H, W >= 11, and a HIP device is present.  Every other call goes to the caller's original function with the caller's arguments.
    `lpips` and `lpips_vgg` are looked up in `evaluation_module` at call time: the caller's networks are used unchanged.

    Limits.  A protocol object that captured `compute_metrics` before the swap keeps the original: `NerfWEvaluationProtocol.__init__` stores
    it as an attribute, so call this first.  `render()` and `image_to_srgb` are not touched: linear colour space, background blending and
    alpha stay the caller's.  Logged values move: SSIM by about 1e-10 and less, MSE / MAE / PSNR by the difference between NumPy's float32
    mean and a float64 sum of the same float32 terms (about 1e-7 relative), which is why this is off unless called."""
    import numpy as np
    original = evaluation_module.compute_metrics

    def covered(pred, gt):
        if not (isinstance(pred, np.ndarray) and isinstance(gt, np.ndarray)):
            return False
        if pred.dtype not in (np.uint8, np.float32) or gt.dtype not in (np.uint8, np.float32):
            return False
        if gt.ndim < 3 or pred.ndim != gt.ndim or pred.shape[:-1] != gt.shape[:-1] or pred.shape[-1] < gt.shape[-1]:
            return False
        if not 1 <= gt.shape[-1] <= 4 or gt.shape[-3] < 11 or gt.shape[-2] < 11 or any(n == 0 for n in gt.shape):
            return False
        return torch.cuda.is_available()

    def compute_metrics(*args, **kwargs):
        if len(args) != 2 or set(kwargs) - {"reduce", "run_lpips_vgg"} or not covered(*args):
            return original(*args, **kwargs)
        import wg_fused_metrics
        return wg_fused_metrics.compute_metrics(*args, **kwargs, lpips=evaluation_module.lpips,
                                                lpips_vgg=getattr(evaluation_module, "lpips_vgg", None))

    compute_metrics.__wrapped__ = original
    evaluation_module.compute_metrics = compute_metrics

    def undo():
        if evaluation_module.compute_metrics is compute_metrics:
            evaluation_module.compute_metrics = original
    return undo


def fuse_evaluation_lpips(evaluation_module):
    """Swap `evaluation_module._lpips` (the reference's wildgaussians/evaluation.py:255-291) for a wrapper over wg_fused_lpips.LPIPS.
    -> a function that puts the original back.  Off unless called.

    `lpips_alex` and `lpips_vgg` look `_lpips` up as a module global when they are called, so the swap reaches the original
    `compute_metrics` and the one `fuse_evaluation_metrics` installs (which is handed `evaluation_module.lpips`) alike, whenever it is made.
    No network is ever constructed here (the caller's constructor downloads its weights): while `evaluation_module._LPIPS_CACHE` has no entry
    for `net`, the call goes to the original function, which builds and caches it.  From then on a covered call -- two float NumPy arrays of
    one shape [..., H, W, 3], version "0.1", a cached module that wg_fused_lpips.structure_covered accepts, H and W at or above the net's
    minimum (31 for alex, 16 for vgg), a HIP device -- is served by a wg_fused_lpips.LPIPS kept beside that cache entry (rebuilt when the entry
    is another object).  Every other call reaches the original with the caller's arguments.  The result is float32, reshaped to the batch
    shape, as the original returns it; values move within float32 rounding, which is why this is off unless called."""
    import numpy as np
    original = evaluation_module._lpips
    fused = {}   # net -> (the cache entry it was built from, wg_fused_lpips.LPIPS or None for an uncovered module)

    def parse(args, kwargs):
        names = ("a", "b", "net", "version")
        if len(args) > len(names) or set(kwargs) - set(names[len(args):]):
            return None
        given = dict(zip(names, args), **kwargs)
        if not all(k in given for k in names[:3]):
            return None
        return given["a"], given["b"], given["net"], given.get("version", "0.1")

    def served_by(a, b, net, version):
        import wg_fused_lpips
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype.kind == "f" and b.dtype.kind == "f"):
            return None
        if a.shape != b.shape or a.ndim < 3 or a.shape[-1] != 3 or a.size == 0 or version != "0.1" or not isinstance(net, str):
            return None
        lp_net = getattr(evaluation_module, "_LPIPS_CACHE", {}).get(net)
        if lp_net is None or not torch.cuda.is_available():
            return None
        entry = fused.get(net)
        if entry is None or entry[0] is not lp_net:
            covered = wg_fused_lpips.structure_covered(lp_net)
            entry = fused[net] = (lp_net, wg_fused_lpips.LPIPS.from_module(lp_net) if covered else None)
        op = entry[1]
        if op is None or min(a.shape[-3], a.shape[-2]) < wg_fused_lpips.MIN_SIDE[op.net]:
            return None
        try:
            op._fresh()   # the module may have left the covered case since (train mode, another dtype)
        except RuntimeError:
            return None
        return op

    def _lpips(*args, **kwargs):
        parsed = parse(args, kwargs)
        op = served_by(*parsed) if parsed is not None else None
        if op is None:
            return original(*args, **kwargs)   # the caller's own code, not a fallback of this library
        a, b = parsed[0], parsed[1]
        batch_shape, img_shape = a.shape[:-3], a.shape[-3:]
        upload = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).view(-1, *img_shape).to(op.device).permute(0, 3, 1, 2)
        ta, tb = upload(a), upload(b)
        if not op.input_covered(ta, tb):
            return original(*args, **kwargs)
        return op(ta, tb).cpu().numpy().reshape(batch_shape)

    _lpips.__wrapped__ = original
    evaluation_module._lpips = _lpips

    def undo():
        if evaluation_module._lpips is _lpips:
            evaluation_module._lpips = original
        fused.clear()
    return undo


def contribution_sweep(trainer, cameras, masks=None):
    """Per-Gaussian contribution statistics of `trainer`'s model over `cameras` -> `diff_gaussian_rasterization.ContributionStats`: for every
    Gaussian the largest blend weight alpha * T any pixel of any of the views gave it, the number of pixels it was blended into and its
    summed weight (what the published pruning criteria are functions of).  One `trainer.render(camera)` per camera under `torch.no_grad()`,
    each inside `collect_contributions`, which feeds the FIRST rasterizer call of the render only (the caller's `_render_internal` makes two
    or three over the same geometry).  `cameras`: anything with `len()` and integer indexing (the trainer's `train_cameras`).  `masks`: None,
    or one bool / float32 [H, W] (or [1, H, W]) tensor or None per camera; pixels whose entry is 0 take no part (the training masks, a
    thresholded uncertainty).  Integer atomics only: two sweeps give the same bits."""
    from diff_gaussian_rasterization import ContributionStats, collect_contributions
    model = trainer.model
    xyz = model.xyz
    n = len(cameras)
    if masks is not None and len(masks) != n:
        raise ValueError("masks must hold one entry (a tensor or None) per camera")
    stats = ContributionStats(xyz.shape[0], xyz.device)
    with torch.no_grad():
        for k in range(n):
            mask = None if masks is None else masks[k]
            if mask is not None and not isinstance(mask, torch.Tensor):
                mask = torch.as_tensor(mask)
            if mask is not None:
                mask = mask.to(xyz.device)
            with collect_contributions(stats, mask):
                trainer.render(cameras[k])
    if stats.views != n:
        raise RuntimeError(f"contribution_sweep: {n} cameras were rendered but {stats.views} frames were collected -- the render did not go "
                           "through diff_gaussian_rasterization.GaussianRasterizer")
    return stats


def prune_by_contribution(trainer, cameras, *, masks=None, **thresholds) -> int:
    """Remove the Gaussians of `trainer`'s model that fail `ContributionStats.keep_mask(**thresholds)` (min_max_weight=, min_hits=,
    min_weight_sum=) over a `contribution_sweep` of `cameras` -> the number removed.  The removal is the model's own: `_prune_points(mask)`
    (or `_prune(mask)` where the model names it so), which shrinks the parameters, the optimizer state and the densification statistics
    together.  Floaters and the leftovers of transient objects -- Gaussians no training view blends with a weight worth keeping, or only in
    masked pixels -- go this way before an export or a fine-tune.  Nothing calls it by default."""
    if not thresholds:
        raise ValueError("prune_by_contribution needs at least one threshold: min_max_weight=, min_hits= or min_weight_sum=")
    model = trainer.model
    prune = getattr(model, "_prune_points", None) or getattr(model, "_prune", None)
    if prune is None:
        raise AttributeError("the model has neither _prune_points nor _prune")
    keep = contribution_sweep(trainer, cameras, masks=masks).keep_mask(**thresholds)
    removed = int((~keep).sum())
    if removed:
        with torch.no_grad():
            prune(~keep)
    return removed
