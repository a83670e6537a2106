#!/usr/bin/env python3
"""What evaluating one test image costs, and how far the fused metrics lie from the oracle, on the same GPU in the same run.

    python scripts/bench_image_metrics.py [--calls 30] [--host-calls 3] [--warmup 3] [--out-dir profiles/image_metrics]

Writes <out-dir>/accuracy.json and <out-dir>/bench.json.

accuracy.json: per case of tests/image_metrics_lib.py the deviation of wg_fused_metrics from the NumPy oracle (SSIM absolute, MSE and MAE
relative), and of wg_fused_metrics.quantize_frame from the NumPy expression (a count of differing bytes).

bench.json: per size (1600x1200, 1920x1080; the full frame and its right half) three legs, alternating call by call, each starting from the
float32 [3, H, W] render on the device and ending with Python floats on the host:

    host_chain      the reference's chain as it runs today: clamp, nan_to_num, permute, the float copy to the host (pageable), the CPU
                    quantisation, then the NumPy restatement of the metrics from tests/image_metrics_lib.py.  That restatement filters all
                    rows at once, which is FASTER than the reference's Python loop of np.convolve over rows: this leg flatters the parent.
                    It is slow, so it runs --host-calls times only (recorded as "calls")
    torch_float64   the same arithmetic as float64 PyTorch operators on the device (conv2d with the separable taps): the fair GPU yardstick
    fused           wg_fused_metrics.frame_metrics on the raw render

Host wall time per call (every leg ends by reading its results, which waits for the device).  Medians with p10 / p90.  Launches and host
synchronisations per call are counted with torch.profiler over one call of each device leg ("not counted" where the profiler is missing).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wild-gaussians_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import image_metrics_lib as L  # noqa: E402

DEV = "cuda:0"


def make_pair(H, W, seed):
    """(render float32 [3, H, W] on the device, gt uint8 [H, W, 3] on the host): a smooth image and a noisy render of it."""
    rng = np.random.default_rng(seed)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    gt = ((np.sin(y / 37.0 + c) + np.cos(x / 53.0 - c)) * 60 + 128 + rng.integers(-8, 9, (H, W, 3))).clip(0, 255).astype(np.uint8)
    render = np.moveaxis(gt.astype(np.float32) / 255.0, -1, 0) + rng.normal(0, 0.02, (3, H, W)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(render)).to(DEV), gt


def host_chain(render, gt, roi):
    frame = torch.clamp(render, 0, 1).nan_to_num_(0).permute(1, 2, 0).cpu().numpy()
    pred = L.quantize(frame)
    a, b = L.normalize(L.to_float32(L.crop(pred, roi))), L.normalize(L.to_float32(L.crop(gt, roi)))
    mse = np.mean((a - b) ** 2, (-3, -2, -1))
    return {"psnr": float(-10 * np.log10(mse)), "ssim": float(np.mean(L.ssim_map(b, a))), "mae": float(np.mean(np.abs(b - a), (-3, -2, -1))),
            "mse": float(mse)}


class TorchFloat64:
    def __init__(self):
        t = torch.from_numpy(L.taps()).to(DEV)
        self.kx, self.ky = t.view(1, 1, 1, -1), t.view(1, 1, -1, 1)

    def blur(self, z):   # [N, 1, h, w] float64, valid windows
        return F.conv2d(F.conv2d(z, self.kx), self.ky)

    def __call__(self, render, gt_dev, roi):
        x = torch.clamp(render, 0, 1).nan_to_num_(0)
        a = (x * 255.0).to(torch.uint8).to(torch.float32) / 255.0                      # [3, H, W]
        b = gt_dev.permute(2, 0, 1).to(torch.float32) / 255.0
        if roi is not None:
            y0, y1, x0, x1 = roi
            a, b = a[:, y0:y1, x0:x1], b[:, y0:y1, x0:x1]
        d = a - b
        mse, mae = (d * d).double().mean(), d.abs().double().mean()
        planes = torch.cat([a, b, a * a, b * b, a * b]).double().unsqueeze(1)          # float32 products, then float64
        mu0, mu1, s00, s11, s01 = self.blur(planes).squeeze(1).split(3)
        mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
        eps = float(np.finfo(np.float32).eps) ** 2
        sigma00, sigma11, sigma01 = (s00 - mu00).clamp_min(eps), (s11 - mu11).clamp_min(eps), s01 - mu01
        sigma01 = torch.sign(sigma01) * torch.minimum(torch.sqrt(sigma00 * sigma11), sigma01.abs())
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        ssim = (((2 * mu01 + c1) * (2 * sigma01 + c2)) / ((mu00 + mu11 + c1) * (sigma00 + sigma11 + c2))).mean()
        mse, mae, ssim = torch.stack([mse, mae, ssim]).cpu().tolist()
        return {"psnr": -10 * np.log10(mse), "ssim": ssim, "mae": mae, "mse": mse}


def stats(ms):
    v = np.sort(np.array(ms))
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "calls": len(ms)}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def count_launches(fn):
    """{"kernel_launches", "memcpy", "host_syncs"} of one call, from torch.profiler's device and runtime events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
        kernels = memcpy = syncs = 0
        for e in prof.events():
            name = e.name
            if str(e.device_type).endswith("CUDA"):
                if "memcpy" in name.lower() or "copy" in name.lower() and "kernel" not in name.lower():
                    memcpy += 1
                else:
                    kernels += 1
            elif name in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMemcpyWithStream", "hipMemcpy"):
                syncs += 1
        return {"kernel_launches": kernels, "memcpy": memcpy, "host_syncs": syncs}
    except Exception as e:   # the profiler is an extra: the timings do not depend on it
        return {"not counted": repr(e)}


def accuracy():
    import wg_fused_metrics as M
    rows = {}
    for c in L.CASES:
        pred, gt = L.make_inputs(c)
        o = L.oracle(c, pred, gt)
        if c["kind"] == "batch":
            got = M.compute_metrics(pred, gt, reduce=False)
        else:
            got = M.frame_metrics(torch.from_numpy(pred).to(DEV) if c["kind"] == "render" else pred, gt, roi=c["roi"])
        rel = lambda k: float(np.max(np.where(o[k] == 0, np.abs(got[k]), np.abs(got[k] - o[k]) / np.where(o[k] == 0, 1, o[k]))))  # noqa: E731
        rows[c["name"]] = {"ssim_abs": float(np.max(np.abs(got["ssim"] - o["ssim"]))), "mse_rel": rel("mse"), "mae_rel": rel("mae")}
    edge = L.edge_floats()
    n = edge.size // 3 * 3
    x = edge[:n].reshape(3, 1, n // 3)
    q = M.quantize_frame(torch.from_numpy(x).to(DEV)).cpu().numpy()
    rows["quantize_edge_floats"] = {"values": int(n), "bytes_that_differ": int((q != L.quantize_render(x)).sum())}
    return {"device": torch.cuda.get_device_name(0), "bounds": {"ssim_abs": 1e-10, "mse_rel": 1e-9, "mae_rel": 1e-9, "quantize": "equal bits"},
            "oracle": "tests/image_metrics_lib.py (NumPy, the reference's operation order and dtypes)", "cases": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "image_metrics"))
    args = ap.parse_args()
    import wg_fused_metrics as M
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "accuracy.json"), "w") as f:
        json.dump(accuracy(), f, indent=1)
    print("accuracy.json written", flush=True)

    yardstick = TorchFloat64()
    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "host_calls": args.host_calls, "warmup": args.warmup,
              "timing": "host wall time per call, every leg ends with its results on the host", "sizes": {}}
    for (W, H) in ((1600, 1200), (1920, 1080)):
        render, gt = make_pair(H, W, seed=W)
        gt_dev = torch.from_numpy(gt).to(DEV)
        for label, roi in (("full", None), ("right_half", (0, H, W // 2, W))):
            legs = {"host_chain": lambda: host_chain(render, gt, roi), "torch_float64": lambda: yardstick(render, gt_dev, roi),
                    "fused": lambda: M.frame_metrics(render, gt_dev, roi=roi)}
            for _ in range(args.warmup):
                legs["torch_float64"](), legs["fused"]()
            times, values = {k: [] for k in legs}, {}
            for i in range(args.calls):
                for k, fn in legs.items():
                    if k == "host_chain" and i >= args.host_calls:
                        continue
                    ms, values[k] = timed(fn)
                    times[k].append(ms)
            row = {k: stats(v) for k, v in times.items()}
            row["values"] = values
            row["fused_minus_host_chain"] = {k: values["fused"][k] - values["host_chain"][k] for k in ("ssim", "mse", "mae", "psnr")}
            row["fused_minus_torch_float64"] = {k: values["fused"][k] - values["torch_float64"][k] for k in ("ssim", "mse", "mae", "psnr")}
            row["per_call"] = {"torch_float64": count_launches(legs["torch_float64"]), "fused": count_launches(legs["fused"])}
            result["sizes"][f"{W}x{H}_{label}"] = row
            print(f"{W}x{H} {label}: " + "  ".join(f"{k} {row[k]['median_ms']:.3f} ms" for k in legs), flush=True)
    with open(os.path.join(args.out_dir, "bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("bench.json written")


if __name__ == "__main__":
    main()
