#!/usr/bin/env python3
"""The uncertainty model's two metrics on one MI355X: the fused wg_fused_ssim.msssim / ssim_down against a float32 PyTorch restatement of
the reference's functions (wildgaussians/method.py:126-187; tests/msssim_lib.py) on the same GPU -- what a caller runs without the
`uncertainty_metrics` opt-in.  Three timed patterns per frame size, fused and torch alternating inside ONE process:

  step        msssim(gt, pred, max_size=400, min_size=80) + ssim_down(gt, pred, max_size=400)       (method.py:368-369, every step)
  msssim      the msssim call alone
  dino_mssim  the "dino+mssim" mode's second call, msssim(gt_down, pred_down, min_size=80) on dino_downsample(max_size=350) images (:400-407)

usage: python scripts/bench_msssim.py [--shapes 1200x1600,1080x1920] [--rounds 7] [--out FILE] [--only fused|torch --calls N]

Times are device events around a window of calls sized to at least half a second, after a warm-up of every pattern; medians and ranges over
`--rounds` alternating rounds.  Launch counts: the fused side's from the plan (levels + 3, or less where a launch is skipped; 3 for
ssim_down), the torch side's counted by torch.profiler over one call ("not measured" where the profiler is unavailable).  The two results are
compared at the timed sizes.  --only: N calls of the step pattern of one side and nothing else, for a `rocprofv3 --kernel-trace --stats` run
of its own.  No GPU: an error, no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import msssim_lib as L  # noqa: E402
import wg_fused_ssim as S  # noqa: E402


def dino_downsample_size(h, w, max_size=350):
    """method.py:190-201."""
    if not (max_size < h or max_size < w):
        return h, w
    scale = min(max_size / h, max_size / w)
    return ((int(h * scale) + 13) // 14) * 14, ((int(w * scale) + 13) // 14) * 14


def fused_launches(H, W, max_size, min_size):
    plan = S.msssim_plan(H, W, max_size, min_size)
    return len(plan) + (plan[0] != (H, W)) + (len(plan) > 1) + 1


def torch_launches(fn):
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


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x1600,1080x1920")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["fused", "torch"], default=None)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim.py needs a HIP device")
    dev = torch.device("cuda", 0)
    rows = []
    with torch.no_grad():
        for shape in a.shapes.split(","):
            H, W = (int(s) for s in shape.split("x"))
            g = torch.Generator().manual_seed(H + W)
            gt = torch.rand(1, 3, H, W, generator=g).to(dev)
            pred = (gt.cpu() * 0.8 + 0.2 * torch.rand(1, 3, H, W, generator=g)).to(dev)
            dh, dw = dino_downsample_size(H, W)
            gt_d, pred_d = (F.interpolate(t, size=(dh, dw), mode="bilinear") for t in (gt, pred))
            patterns = {
                "step": (lambda: (S.msssim(gt, pred, max_size=400, min_size=80), S.ssim_down(gt, pred, max_size=400)),
                         lambda: (L.ref_msssim(gt, pred, max_size=400, min_size=80), L.ref_ssim_down(gt, pred, max_size=400))),
                "msssim": (lambda: (S.msssim(gt, pred, max_size=400, min_size=80),),
                           lambda: (L.ref_msssim(gt, pred, max_size=400, min_size=80),)),
                "dino_mssim": (lambda: (S.msssim(gt_d, pred_d, min_size=80),), lambda: (L.ref_msssim(gt_d, pred_d, min_size=80),)),
            }
            if a.only:
                fn = patterns["step"][0 if a.only == "fused" else 1]
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                continue
            launches = {"step": fused_launches(H, W, 400, 80) + 3, "msssim": fused_launches(H, W, 400, 80),
                        "dino_mssim": fused_launches(dh, dw, None, 80)}
            row = {"H": H, "W": W, "msssim_levels": S.msssim_plan(H, W, 400, 80), "dino_mssim_levels": S.msssim_plan(dh, dw, None, 80),
                   "patterns": {}}
            for name, (fused, ref) in patterns.items():
                for _ in range(5):   # warm-up of both sides at this shape
                    out_f, out_r = fused(), ref()
                torch.cuda.synchronize()
                diff = max((x - y).abs().max().item() for x, y in zip(out_f, out_r))
                n_f = max(10, int(500.0 / max(event_ms(fused, 10), 1e-3)) + 1)
                n_r = max(10, int(500.0 / max(event_ms(ref, 10), 1e-3)) + 1)
                tf, tr = [], []
                for _ in range(a.rounds):
                    tf.append(event_ms(fused, n_f))
                    tr.append(event_ms(ref, n_r))
                sf, sr = stats(tf), stats(tr)
                row["patterns"][name] = {"fused": dict(sf, calls_per_window=n_f, launches=launches[name]),
                                         "torch": dict(sr, calls_per_window=n_r, launches=torch_launches(ref)),
                                         "torch_over_fused": round(sr["median_ms"] / sf["median_ms"], 2),
                                         "max_abs_diff_fused_vs_torch_float32": diff}
            rows.append(row)
    if a.only:
        return
    line = {"metric": "msssim_ssim_down", "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
            "timing": "device events around a window of calls of at least 0.5 s; fused and torch alternate per round",
            "baseline": "float32 PyTorch restatement of the reference's msssim / ssim_down on the same GPU", "shapes": rows}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
