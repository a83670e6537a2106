#!/usr/bin/env python3
"""UncertaintyModel._compute_losses around the backbone on one MI355X: the fused wg_fused_uncertainty.compute_losses against a float32
PyTorch restatement of the reference's sequence (wildgaussians/method.py:363-433) on the same GPU -- what a caller runs without the
`uncertainty_loss` opt-in.  Three legs per frame size, alternating inside ONE process, forward + backward each:

  (a) fused     compute_losses with the features precomputed (the model's _get_dino_cached hands them over; all three prepare launches run,
                as they do with the reference's cache, whose lookups never hit)
  (b) torch     the restatement with the same precomputed features: three normalise / pad / resize chains, dropout2d, SyncBatchNorm, the 1x1
                convolution, softplus, the interpolations, the reductions and seven .item() calls.  `uncertainty_metrics` is fused in BOTH legs
  (c) fused+bb  one compute_losses call including tests/uncertainty_lib.py's stand-in backbone (three calls of it), for orientation only: the
                stand-in is a float64 matrix product, not DINOv2

usage: python scripts/bench_uncertainty_step.py [--shapes 1200x1600,1080x1920] [--samples 30] [--out FILE]

Times are device events around each call (the window includes the host round trips a leg makes), median / p10 / p90 of `--samples` calls after a
warm-up of every leg at every shape.  Launch counts come from torch.profiler over one call, host synchronisations from wrapping Tensor.item /
.cpu / .tolist, peak memory from the allocator's peak above what is allocated before the call.  Leg (b) is the yardstick, never the code under
test.  The real model keeps its feature cache on the CPU and copies a cached map to the device on every step; both timed legs leave that copy
out.  No GPU: an error, no fallback."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import uncertainty_lib as L  # noqa: E402
import wg_fused_ssim as S  # noqa: E402
import wg_fused_uncertainty as U  # noqa: E402


class PrecomputedModel(L.StandInModel):
    """_get_dino_cached returns features computed before the timed region: by input shape, and by whether a cache entry is named (the
    prediction's call names none)."""

    def precompute(self, gt, pred):
        g = U.Geometry(gt.shape[2], gt.shape[3], self.patch_size)
        mean, std = self.img_norm_mean, self.img_norm_std
        run = lambda x: self.backbone.get_intermediate_layers(x, n=[self.backbone.num_heads - 1], reshape=True)[-1]
        full, gd, pd = L.prep(gt, mean, std, g.H, g.W), L.prep(gt, mean, std, g.nh, g.nw), L.prep(pred, mean, std, g.nh, g.nw)
        self.pre = {(tuple(full.shape), True): run(full), (tuple(gd.shape), True): run(gd), (tuple(pd.shape), False): run(pd)}

    def _get_dino_cached(self, x, cache_entry=None):
        return self.pre[(tuple(x.shape), cache_entry is not None)]


def torch_compute_losses(model, gt, prediction, prefix="", _cache_entry=None):
    """The reference's sequence for uncertainty_mode == "dino", uncertainty_dino_max_size None, restated in float32 PyTorch."""
    cfg, P = model.config, model.patch_size
    mean, std = model.img_norm_mean[None, :, None, None], model.img_norm_std[None, :, None, None]

    def norm_pad(img):
        (pt, pb), (pl, pr) = U.pads(img.shape[2], P), U.pads(img.shape[3], P)
        return F.pad((img - mean) / std, (pl, pr, pt, pb)), pt, pl

    def down(t):
        nh, nw = U.down_size(*t.shape[2:])
        return t if (nh, nw) == tuple(t.shape[2:]) else F.interpolate(t, size=(nh, nw), mode="bilinear")
    H, W = gt.shape[2:]
    x, pt, pl = norm_pad(gt)
    feat = model._get_dino_cached(x, _cache_entry)
    feat = F.dropout2d(feat, p=cfg.uncertainty_dropout, training=model.training)
    logits = model.conv_seg(model.bn(feat)) + math.log(math.exp(1) - 1)
    u = F.interpolate(F.softplus(logits), size=x.shape[2:], mode="bilinear", align_corners=False).clamp(min=cfg.uncertainty_clip_min)
    u = u[:, :, pt:pt + H, pl:pl + W]
    log_u = torch.log(u)
    ssim_map = S.ssim_down(gt, prediction, max_size=400).unsqueeze(1)
    msssim_map = S.msssim(gt, prediction, max_size=400, min_size=80).unsqueeze(1)
    loss_mult = 1 / (2 * u.pow(2))
    gt_down, pred_down = down(gt), down(prediction)
    xd, dpt, dpl = norm_pad(gt_down)
    yd, _, _ = norm_pad(pred_down)
    with torch.no_grad():
        fx, fy = model._get_dino_cached(xd, _cache_entry), model._get_dino_cached(yd, None)
    cos = F.cosine_similarity(fx, fy, dim=1).unsqueeze(1)
    cos = F.interpolate(cos, size=xd.shape[2:], mode="bilinear", align_corners=False)
    cos = cos[:, :, dpt:dpt + gt_down.shape[2], dpl:dpl + gt_down.shape[3]].detach()
    dino_part = (1 - cos.sub(0.5).div(0.5)).clip(0.0, 1)
    uncertainty_loss = dino_part * down(loss_mult)
    loss_mult = loss_mult.clamp_max(3)
    beta = log_u.mean()
    loss = uncertainty_loss.mean() + cfg.uncertainty_regularizer_weight * beta
    ssim_discounted = (ssim_map * loss_mult).sum() / loss_mult.sum()
    mse_discounted = (torch.pow(gt - prediction, 2) * loss_mult).sum() / loss_mult.sum()
    psnr_discounted = 10 * torch.log10(1 / mse_discounted)
    metrics = {f"{prefix}loss": loss.item(), f"{prefix}ssim": ssim_map.mean().item(), f"{prefix}msssim": msssim_map.mean().item(),
               f"{prefix}ssim_discounted": ssim_discounted.item(), f"{prefix}mse_discounted": mse_discounted.item(),
               f"{prefix}psnr_discounted": psnr_discounted.item(), f"{prefix}beta": beta.item()}
    return loss, metrics, loss_mult.detach()


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or "not measured"
    except Exception as ex:  # noqa: BLE001
        return "not measured (%s)" % type(ex).__name__


def host_syncs(fn):
    count = [0]
    saved = {n: getattr(torch.Tensor, n) for n in ("item", "cpu", "tolist")}

    def wrap(orig):
        def counted(self, *a, **k):
            count[0] += bool(self.is_cuda)
            return orig(self, *a, **k)
        return counted
    try:
        for n, orig in saved.items():
            setattr(torch.Tensor, n, wrap(orig))
        fn()
    finally:
        for n, orig in saved.items():
            setattr(torch.Tensor, n, orig)
    return count[0]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    q = lambda f: round(v[min(len(v) - 1, int(f * len(v)))], 4)
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x1600,1080x1920")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--channels", type=int, default=384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty_step.py needs a HIP device")
    dev = torch.device("cuda", 0)
    rows = []
    for shape in a.shapes.split(","):
        H, W = (int(s) for s in shape.split("x"))
        case = {"name": shape, "H": H, "W": W, "C": a.channels, "training": True, "init": "clamp", "steps": 1, "seed": H + W}
        gt, pred = (t.to(dev) for t in L.make_images(case))
        models = {"a": PrecomputedModel(case).to(dev), "b": PrecomputedModel(case).to(dev), "c": L.StandInModel(case).to(dev)}
        for m in (models["a"], models["b"]):
            m.precompute(gt, pred)

        def leg(name):
            m = models[name]
            m.zero_grad()
            if name == "b":
                loss, metrics, loss_mult = torch_compute_losses(m, gt, pred, "", _cache_entry="k")
            else:
                loss, metrics, loss_mult = U.compute_losses(m, gt, pred, "", _cache_entry="k" if name == "a" else None)
            loss.backward()
            return loss, metrics, loss_mult
        legs = {n: (lambda n=n: leg(n)) for n in "abc"}
        for _ in range(3):   # warm-up of every leg at this shape
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        # the legs draw different dropout masks, so only what does not depend on the mask is compared
        times = {n: [] for n in legs}
        for _ in range(a.samples):
            for n, fn in legs.items():
                times[n].append(event_ms(fn))
        g = U.Geometry(H, W, L.PATCH)
        row = {"H": H, "W": W, "C": a.channels, "feature_map": [a.channels, g.hp, g.wp], "downsampled": [g.nh, g.nw], "legs": {}}
        for n, label in (("a", "fused compute_losses, features precomputed"), ("b", "float32 PyTorch restatement, features precomputed"),
                         ("c", "fused compute_losses including the stand-in backbone")):
            row["legs"][n] = dict(stats(times[n]), what=label, launches=launches(legs[n]), host_syncs=host_syncs(legs[n]),
                                  peak_mb_above_inputs=peak_mb(legs[n]))
        row["torch_over_fused"] = round(row["legs"]["b"]["median_ms"] / row["legs"]["a"]["median_ms"], 2)
        # same mask for both legs: the results compared at the timed size
        kd = U.draw_dropout_factors(a.channels, 0.5, True, dev)
        saved, saved_f = U.draw_dropout_factors, F.dropout2d
        try:
            U.draw_dropout_factors = lambda *args: kd
            F.dropout2d = lambda x, p=0.5, training=True, inplace=False: x * kd.reshape(1, -1, 1, 1)
            models["b"].load_state_dict(models["a"].state_dict())
            la, ma, ua = leg("a")
            lb, mb, ub = leg("b")
        finally:
            U.draw_dropout_factors, F.dropout2d = saved, saved_f
        row["fused_vs_torch_same_mask"] = {"loss": [ma["loss"], mb["loss"]], "max_abs_diff_loss_mult": (ua - ub).abs().max().item(),
                                           "max_abs_diff_metrics": max(abs(ma[k] - mb[k]) for k in ma),
                                           "max_rel_diff_conv_weight_grad": ((models["a"].conv_seg.weight.grad - models["b"].conv_seg.weight.grad).abs().max()
                                                                             / models["b"].conv_seg.weight.grad.abs().max()).item()}
        rows.append(row)
    line = {"metric": "uncertainty_step", "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
            "timing": "device events around each call, forward + backward; legs alternate call by call; median / p10 / p90",
            "baseline": "leg b: float32 PyTorch restatement of the reference's sequence on the same GPU, msssim / ssim_down fused in both legs",
            "not_included": "the backbone (legs a, b), the host-to-device copy of cached features", "shapes": rows}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
