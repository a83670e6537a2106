#!/usr/bin/env python3
"""LPIPS v0.1 (AlexNet and VGG16 trunks) of one image pair on one MI355X: wg_fused_lpips.LPIPS against float32 PyTorch on the same GPU, with the
generated weights of tests/lpips_lib.py (timing does not depend on the weights' values).  Three legs per net and shape, alternating call by
call inside ONE process:

  (a) fused           LPIPS.from_module(module)(pred, gt) from device tensors [1, 3, H, W]
  (b) torch module    the float32 stand-in of the caller's module (the reference's layer sequence, the framework's convolution library) on the
                      same device tensors, fed as the caller feeds it (clip, * 2 - 1): the yardstick for the kernels
  (c) caller's path   `_lpips(a, b, net)` from NumPy arrays [H, W, 3], upload included: the stand-in evaluation module's own function (c_torch)
                      against the function wg_integration.fuse_evaluation_lpips swaps in (c_fused)

usage: python scripts/bench_lpips.py [--shapes 1200x1600,1080x1920] [--nets alex,vgg] [--samples 30] [--out FILE]

Times of (a) and (b) are device events around each call, of (c) host wall time around the call (it ends with a device-to-host copy); median /
p10 / p90 of `--samples` calls after a warm-up of every leg.  The FIRST call of legs (a) and (b) at a new image size is recorded separately, on
a size no earlier call has seen (phototourism test images all differ in size): host wall time with a device synchronise.  Launch counts come
from torch.profiler over one call, peak memory from the allocator's peak above what is allocated before the call (for (a) the operator's
scratch is dropped first, so that it counts; the operator behind c_fused keeps its own between calls, so that figure leaves it out), the fraction of the float32 MFMA peak (157 TFLOP/s) from the counted multiply-adds of the two
images' convolutions over the median.  The accuracy record, every gated quantity as a ratio of max(ref32_dev, 16 ulps), is written by
tests/test_lpips.py under WG_RECORD=1 (profiles/lpips/accuracy.json).  No GPU: an error, no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lpips_lib as L  # noqa: E402
import wg_fused_lpips as D  # noqa: E402
import wg_integration  # noqa: E402

PEAK_TFLOPS = 157.0


def conv_macs(net, H, W):
    """Multiply-adds of the trunk's convolutions for ONE image."""
    h, w, total = H, W, 0
    for cin, cout, k, s, p, pool_w, _ in D.CONVS[D.NET_OF[net]]:
        if pool_w:
            h, w = (h - pool_w) // 2 + 1, (w - pool_w) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += h * w * cout * cin * k * k
    return total


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


def peak_mb(fn, before_fn=None):
    if before_fn is not None:
        before_fn()
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
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = sorted(v)
    q = lambda f: round(v[min(len(v) - 1, int(f * len(v)))], 4)
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x1600,1080x1920")
    ap.add_argument("--nets", default="alex,vgg")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py needs a HIP device")
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    result = {"metric": "lpips_ms", "device": torch.cuda.get_device_name(0), "samples": args.samples, "peak_tflops_f32_mfma": PEAK_TFLOPS,
              "legs": {"a": "fused, device tensors", "b": "float32 torch module of the reference's shape, device tensors",
                       "c_torch": "the caller's _lpips from NumPy arrays, upload included", "c_fused": "the swapped _lpips from NumPy arrays, upload included"},
              "nets": {}}
    for net in args.nets.split(","):
        ev = L.stand_in_evaluation_module(nets=(net,))
        module = ev._LPIPS_CACHE[net].to(dev)
        fused = D.LPIPS.from_module(module)
        original_lpips = ev._lpips
        undo = wg_integration.fuse_evaluation_lpips(ev)
        swapped_lpips = ev._lpips
        result["nets"][net] = {}
        for H, W in shapes:
            rng = np.random.default_rng(H * W)
            a_np, b_np = rng.random((H, W, 3), dtype=np.float32), rng.random((H, W, 3), dtype=np.float32)
            pred = torch.from_numpy(a_np).to(dev).permute(2, 0, 1)[None]
            gt = torch.from_numpy(b_np).to(dev).permute(2, 0, 1)[None]
            torch_leg = lambda p=pred, g=gt: module(p.clamp(0, 1).mul(2).sub(1), g.clamp(0, 1).mul(2).sub(1))
            legs = {"a": (lambda p=pred, g=gt: fused(p, g), event_ms), "b": (torch_leg, event_ms),
                    "c_torch": (lambda: original_lpips(a_np, b_np, net), wall_ms), "c_fused": (lambda: swapped_lpips(a_np, b_np, net), wall_ms)}
            entry = {}
            with torch.no_grad():
                # the first call at a size nothing has seen yet: one row more than the shape that is measured
                odd = [torch.rand(1, 3, H + 1, W, device=dev) for _ in range(2)]
                entry["first_call_at_a_new_size_ms"] = {
                    "a": round(wall_ms(lambda: fused(odd[0], odd[1])), 3),
                    "b": round(wall_ms(lambda: module(odd[0].clamp(0, 1).mul(2).sub(1), odd[1].clamp(0, 1).mul(2).sub(1))), 3)}
                del odd
                for fn, _ in legs.values():   # warm-up of every leg
                    fn()
                    fn()
                torch.cuda.synchronize()
                times = {k: [] for k in legs}
                for _ in range(args.samples):
                    for k, (fn, clock) in legs.items():
                        times[k].append(clock(fn))
                for k, v in times.items():
                    entry[k] = dict(stats(v), launches=launches(legs[k][0]),
                                    peak_mb_above_inputs=peak_mb(legs[k][0], (lambda: setattr(fused, "_scratch", None)) if k in ("a", "c_fused") else None))
                values = {k: float(np.asarray(fn().cpu() if torch.is_tensor(fn()) else fn()).reshape(-1)[0]) for k, (fn, _) in legs.items()}
            macs = 2 * conv_macs(net, H, W)
            entry.update({"gflop_two_images": round(2 * macs / 1e9, 1), "scratch_mb": round(D.scratch_floats(fused.net, 1, H, W) * 4 / 2 ** 20, 1),
                          "values": values,
                          "fraction_of_f32_mfma_peak": {k: round(2 * macs / (entry[k]["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12), 4) for k in ("a", "b")}})
            result["nets"][net][f"{H}x{W}"] = entry
            print(net, f"{H}x{W}", json.dumps(entry), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:   # after every shape: a later shape that runs out of time or memory leaves the earlier ones
                json.dump(result, f, indent=1, sort_keys=True)
            del pred, gt, legs, torch_leg
            fused._scratch = None
            torch.cuda.empty_cache()
        undo()
        del fused, module, ev
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
