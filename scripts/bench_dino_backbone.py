#!/usr/bin/env python3
"""The frozen DINOv2 ViT-S/14 backbone of the uncertainty model on one MI355X: wg_fused_dino.DinoFeatures against float32 PyTorch on the same
GPU, with the generated weights of tests/dino_lib.py (timing does not depend on the weights' values).  Three legs per shape, alternating call
by call inside ONE process:

  (a) fused        DinoFeatures(backbone).features(x): blocks 0..5, attention with an online softmax, no N x N tensor
  (b) torch today  a torch restatement of what the caller runs: all 12 blocks, attention materialised (softmax(q k^T) as a [6, N, N] tensor)
  (c) torch 6+sdpa the restatement stopped after block 5, with F.scaled_dot_product_attention: the honest yardstick for the kernels themselves

usage: python scripts/bench_dino_backbone.py [--shapes 1204x1610,1092x1932,266x350] [--samples 30] [--out FILE]

Shapes are backbone inputs [1, 3, H, W] (a 1600x1200 frame padded to 1610x1204, a 1920x1080 one to 1932x1092, the 350-pixel pass); the smallest
shape is also run as B = 2 against two B = 1 calls.  Times are device events around each call, median / p10 / p90 of `--samples` calls after a
warm-up of every leg at every shape.  Launch counts come from torch.profiler over one call, peak memory from the allocator's peak above what is
allocated before the call, the fraction of the float32 MFMA peak (157 TFLOP/s) from the 6-block operation count over leg (a)'s median, and
every leg's max |. - float64 oracle| on the smallest shape from tests/dino_lib.oracle_features.  No GPU: an error, no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dino_lib as L  # noqa: E402
import wg_fused_dino as D  # noqa: E402

PEAK_TFLOPS = 157.0


def flops(H, W, blocks, B=1):
    n_patch = (H // 14) * (W // 14)
    N = 5 + n_patch
    linear = 2 * (384 * 1152 + 384 * 384 + 2 * 384 * 1536) * N
    attention = 4 * N * N * 384
    return B * (2 * 588 * 384 * n_patch + blocks * (linear + attention))


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
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    q = lambda f: round(v[min(len(v) - 1, int(f * len(v)))], 4)
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1204x1610,1092x1932,266x350")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_backbone", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino_backbone.py needs a HIP device")
    dev = torch.device("cuda", 0)
    weights = L.make_weights()
    today = L.TorchBackbone(weights, conv=True).to(dev)                                   # (b); also the module the fused extractor reads
    yard = L.TorchBackbone(weights, stop_early=True, sdpa=True, conv=True).to(dev)        # (c)
    fused = D.DinoFeatures(today)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    small = min(shapes, key=lambda s: s[0] * s[1])
    result = {"metric": "dino_backbone_ms", "device": torch.cuda.get_device_name(0), "samples": args.samples, "peak_tflops_f32_mfma": PEAK_TFLOPS,
              "legs": {"a": "fused, blocks 0..5", "b": "torch, 12 blocks, materialised attention", "c": "torch, blocks 0..5, scaled_dot_product_attention"},
              "shapes": {}}

    def legs_for(x):
        take = [today.num_heads - 1]
        return {"a": lambda: fused.features(x),
                "b": lambda: today.get_intermediate_layers(x, n=take, reshape=True)[-1],
                "c": lambda: yard.get_intermediate_layers(x, n=take, reshape=True)[-1]}

    def measure(name, legs, extra):
        with torch.no_grad():
            for fn in legs.values():   # warm-up of every leg
                fn()
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in legs}
            for _ in range(args.samples):
                for k, fn in legs.items():
                    times[k].append(event_ms(fn))
            entry = {k: dict(stats(v), launches=launches(legs[k]), peak_mb_above_inputs=peak_mb(legs[k])) for k, v in times.items()}
        entry.update(extra)
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        return entry

    for H, W in shapes:
        x = torch.from_numpy(np.random.default_rng(H * W).standard_normal((1, 3, H, W)).astype(np.float32)).to(dev)
        e = measure(f"1x3x{H}x{W}", legs_for(x), {"tokens": 5 + (H // 14) * (W // 14), "gflop_6_blocks": round(flops(H, W, 6) / 1e9, 1),
                                                  "gflop_12_blocks": round(flops(H, W, 12) / 1e9, 1)})
        e["fraction_of_f32_mfma_peak"] = {"a": round(flops(H, W, 6) / (e["a"]["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12), 4),
                                          "c": round(flops(H, W, 6) / (e["c"]["median_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12), 4)}
        print("   fraction of peak", e["fraction_of_f32_mfma_peak"], flush=True)

    # the smallest shape as a batch of two against two single calls (the two 350-pixel passes of a step)
    H, W = small
    x2 = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 3, H, W)).astype(np.float32)).to(dev)
    measure(f"2x3x{H}x{W}", {"a_batch": lambda: fused.features(x2),
                             "a_two_calls": lambda: (fused.features(x2[:1]), fused.features(x2[1:])),
                             "c_two_calls": lambda: (yard.get_intermediate_layers(x2[:1], n=[5], reshape=True), yard.get_intermediate_layers(x2[1:], n=[5], reshape=True))},
            {"tokens": 5 + (H // 14) * (W // 14)})

    # every leg against the float64 oracle on the smallest shape
    xs = torch.from_numpy(np.random.default_rng(11).standard_normal((1, 3, H, W)).astype(np.float32))
    ref = L.oracle_features(weights, xs).numpy()
    with torch.no_grad():
        result["max_abs_error_vs_float64"] = {"shape": f"1x3x{H}x{W}", "largest_magnitude": float(np.abs(ref).max()),
                                              **{k: float(np.abs(fn().cpu().double().numpy() - ref).max()) for k, fn in legs_for(xs.to(dev)).items()}}
    print("errors", result["max_abs_error_vs_float64"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
