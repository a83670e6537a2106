#!/usr/bin/env python3
"""The appearance MLP on one MI355X: wg_fused_gaussians.appearance_mlp against the reference's formulation (wildgaussians/method.py:896-897:
`torch.cat`, the nn.Sequential, `* 0.01`, autograd's backward pass) on the same GPU, in ONE process, the two legs alternating.

usage: python scripts/bench_appearance_mlp.py [--rows 1000000,3000000] [--samples 30] [--out FILE] [--commit ID] [--accuracy FILE]

Per size (widths 3 + 24 + 32; colour a stride-48 view of the features) and per form of the appearance embedding (per row [P, 32] / shared
[32]; the torch leg always sees the per-row form, which is what the reference's caller builds): forward alone (no_grad) and forward +
backward with a fixed cotangent and gradients to all inputs and weights.  Every call is timed by its own pair of device events after a
warm-up of both legs; legs alternate in blocks of five calls; median, p10 and p90 over --samples calls.  Launches are counted by
torch.profiler over one call; peak memory is torch.cuda.max_memory_allocated over one forward + backward above what is allocated before it
(inputs and weights).  --accuracy: per tensor max(err / bound) against the float64 oracle of tests/appearance_mlp_lib.py for the fused
operator and for PyTorch's float32 on the same device, and their ratio (recorded, not gated).  No GPU: an error, no fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import appearance_mlp_lib as L  # noqa: E402
import wg_fused_gaussians as FG  # noqa: E402

G, E = 24, 32
MACS_PER_ROW = 98048   # forward + recompute + both gradient products at K = 59 (the issue's count)


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


def one_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    return {"median_ms": round(q(0.5), 4), "p10_ms": round(q(0.1), 4), "p90_ms": round(q(0.9), 4), "samples": len(v)}


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_size(P, shared, samples, dev):
    g = torch.Generator().manual_seed(P + shared)
    feats = torch.rand(P, 48, generator=g).to(dev).requires_grad_(True)
    gemb = (torch.rand(P, G, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    avec = (torch.randn(E, generator=g) * 0.3).to(dev)
    arow = avec[None].repeat(P, 1).requires_grad_(True)
    avec.requires_grad_(True)
    W = [w.to(dev).requires_grad_(True) for w in L.draw_weights(3 + G + E, 1)]
    mlp = torch.nn.Sequential(torch.nn.Linear(59, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(), torch.nn.Linear(128, 6)).to(dev)
    with torch.no_grad():
        for p, w in zip(mlp.parameters(), W):
            p.copy_(w)
    cot = torch.randn(P, 6, generator=g).to(dev)
    params = list(mlp.parameters())

    def torch_fwd():
        return mlp(torch.cat((feats[..., :3], gemb, arow), dim=-1)) * 0.01

    def fused_fwd():
        if shared:
            return FG.appearance_mlp((feats[..., :3], gemb), W, shared=avec)
        return FG.appearance_mlp((feats[..., :3], gemb, arow), W)

    def torch_fb():
        return torch.autograd.grad(torch_fwd(), [feats, gemb, arow] + params, cot)

    def fused_fb():
        return torch.autograd.grad(fused_fwd(), [feats, gemb, avec if shared else arow] + W, cot)

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    row = {"P": P, "aembedding": "shared [32]" if shared else "per row [P, 32]", "patterns": {}}
    for name, fused, ref in (("forward", nograd(fused_fwd), nograd(torch_fwd)), ("forward_backward", fused_fb, torch_fb)):
        for _ in range(3):
            of, orf = fused(), ref()
        torch.cuda.synchronize()
        first = (lambda o: o if torch.is_tensor(o) else o[0])
        diff = float((first(of) - first(orf)).abs().max())
        del of, orf
        tf, tr = [], []
        while len(tf) < samples:
            tf += [one_ms(fused) for _ in range(5)]
            tr += [one_ms(ref) for _ in range(5)]
        sf, sr = stats(tf), stats(tr)
        row["patterns"][name] = {"fused": dict(sf, launches=launches(fused)), "torch": dict(sr, launches=launches(ref)),
                                 "torch_over_fused_median": round(sr["median_ms"] / sf["median_ms"], 3),
                                 "max_abs_diff_first_output": diff}
    row["peak_bytes_above_inputs"] = {"fused": peak_above_inputs(fused_fb), "torch": peak_above_inputs(torch_fb)}
    fb = row["patterns"]["forward_backward"]["fused"]["median_ms"]
    row["fused_forward_backward_tflops"] = round(2 * MACS_PER_ROW * P / (fb * 1e-3) / 1e12, 2)
    return row


def accuracy(dev):
    """max(err / bound) per tensor: the fused operator and PyTorch's float32 on this device, against the float64 oracle."""
    rows = []
    for P, shared in ((357, False), (357, True), (33000, False), (33000, True)):
        c = L.make_case(P, G, E, 77 + P)
        cot = L.dense_cotangent(P, 77 + P)
        o = L.oracle(c, cot)
        feats = c["features"].to(dev)
        res = {}
        for leg in ("fused", "torch"):
            colour = feats[:, :3].detach().requires_grad_(True)
            gemb = c["gemb"].to(dev).requires_grad_(True)
            W = [w.to(dev).requires_grad_(True) for w in c["weights"]]
            arow = c["aemb"][None].repeat(P, 1).to(dev).requires_grad_(True)
            avec = c["aemb"].to(dev).requires_grad_(True)
            if leg == "fused" and shared:
                out = FG.appearance_mlp((colour, gemb), W, shared=avec)
            elif leg == "fused":
                out = FG.appearance_mlp((colour, gemb, arow), W)
            else:
                x = torch.cat((colour, gemb, arow), dim=-1)
                out = (torch.relu(torch.relu(x @ W[0].t() + W[1]) @ W[2].t() + W[3]) @ W[4].t() + W[5]) * 0.01
            out.backward(cot.to(dev))
            got = {"out": out.detach(), "dx": torch.cat([colour.grad, gemb.grad], 1),
                   "dshared": avec.grad if (leg == "fused" and shared) else arow.grad.sum(0)}
            got.update({n: w.grad for n, w in zip(["dW1", "db1", "dW2", "db2", "dW3", "db3"], W)})
            res[leg] = {}
            for k, v in got.items():
                want, bound = o[k], o["e_" + k]
                if k == "dx":
                    want, bound = want[:, :3 + G], bound[:, :3 + G]
                res[leg][k] = L.ratio(v, want, bound)
        rows.append({"P": P, "aembedding": "shared" if shared else "per row", "discarded_candidates": round(c["discarded"], 4),
                     "fused_err_over_bound": {k: round(v, 4) for k, v in res["fused"].items()},
                     "torch_float32_err_over_bound": {k: round(v, 4) for k, v in res["torch"].items()},
                     "fused_over_torch": {k: (round(res["fused"][k] / res["torch"][k], 3) if res["torch"][k] > 0 else None) for k in res["fused"]}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,3000000")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--accuracy", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_appearance_mlp.py needs a HIP device")
    dev = torch.device("cuda", 0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    head = {"device": torch.cuda.get_device_name(0), "commit": commit, "arguments": {"rows": a.rows, "samples": a.samples}}
    if a.accuracy:
        acc = dict(head, metric="appearance_mlp_accuracy", yardstick="max over elements of |result - float64| / a-priori float32 rounding bound "
                   "(tests/appearance_mlp_lib.py); recorded, not gated", cases=accuracy(dev))
        os.makedirs(os.path.dirname(os.path.abspath(a.accuracy)), exist_ok=True)
        with open(a.accuracy, "w") as f:
            json.dump(acc, f, indent=1)
        print(json.dumps(acc))
    rows = []
    for P in (int(s) for s in a.rows.split(",") if s):
        for shared in (False, True):
            rows.append(bench_size(P, shared, a.samples, dev))
            torch.cuda.empty_cache()
    line = dict(head, metric="appearance_mlp", widths="3 + 24 + 32 -> 128 -> 128 -> 6",
                timing="one pair of device events per call after a warm-up; legs alternate in blocks of five calls; median / p10 / p90",
                baseline="torch.cat + nn.Sequential + * 0.01 and autograd's backward on the same GPU, per-row aembedding",
                macs_per_row_forward_backward=MACS_PER_ROW, sizes=rows)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
