#!/usr/bin/env python3
"""Writes tests/golden/uncertainty_ref.npz: what the REFERENCE's own UncertaintyModel._compute_losses (wildgaussians/method.py:204-433, with
dino_downsample, ssim, ssim_down, _ssim_parts and msssim) returns on the cases of tests/uncertainty_lib.py, on the CPU.

    python tests/golden/make_uncertainty_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies.  As make_msssim_golden.py does, the class and the five functions are executed out of
method.py (the module itself needs packages a test machine may lack).  The name `dinov2` in that namespace is a stub whose
dinov2_vits14_reg(pretrained=True) returns tests/uncertainty_lib.StandInBackbone: the real module and its weights are never reached.
`F` in that namespace forwards to torch.nn.functional, except that dropout2d records the channel factors it drew (float32 run) or applies
the recorded ones (float64 run), and softplus records its output (the tensor `s`).

The fixture holds recorded data only.  Per case: the reference's float32 outputs, its outputs on the same inputs, parameters and dropout
factors in float64, ref32_dev = max |float32 - float64| per tensor (over the whole tensor), the dropout factors of every step, the keys of
`_images_cache` after the last step, and the float64 oracle's clamp margin min |bilinear(s) - clip_min|, which the generator holds above
1e-5 (the clamp's derivative is discontinuous there).  loss_mult is stored on a strided grid (uncertainty_lib.sample_stride) to respect
the size limit of a committed file.  Inputs and parameters are regenerated from the seeds by tests/uncertainty_lib.py.
"""
import itertools
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import uncertainty_lib as L  # noqa: E402


class RecordingF:
    """torch.nn.functional with a recording / replaying dropout2d and a recording softplus."""

    def __init__(self):
        self.factors, self.replay, self.softplus_out = [], None, None

    def __getattr__(self, name):
        return getattr(F, name)

    def dropout2d(self, x, p=0.5, training=True, inplace=False):
        if self.replay is not None:
            k = self.replay[len(self.factors)]
            self.factors.append(k)
            return x * torch.as_tensor(k, dtype=x.dtype).reshape(1, -1, 1, 1)
        out = F.dropout2d(x, p=p, training=training)
        flat_x, flat_o = x.reshape(x.shape[1], -1), out.reshape(x.shape[1], -1)
        at = flat_x.abs().argmax(1, keepdim=True)
        self.factors.append((flat_o.gather(1, at) / flat_x.gather(1, at)).reshape(-1).double().round(decimals=6).numpy())
        return out

    def softplus(self, x, *a, **k):
        self.softplus_out = F.softplus(x, *a, **k)
        return self.softplus_out


def reference_namespace(checkout, case, rf):
    src = open(os.path.join(checkout, "wildgaussians", "method.py")).read()
    stub = types.SimpleNamespace(dinov2_vits14_reg=lambda pretrained=True: L.StandInBackbone(case["C"], case["seed"] + 3))
    ns = {"torch": torch, "F": rf, "math": math, "nn": nn, "Tensor": Tensor, "itertools": itertools, "np": np, "Optional": __import__("typing").Optional,
          "Config": object, "dinov2": stub, "assert_not_none": lambda v: v}
    for head in ("def ssim(img1, img2, window_size=11, size_average=True):", "def ssim_down(x, y, max_size=None):",
                 "def _ssim_parts(img1, img2, window_size=11):", "def msssim(x, y, max_size=None, min_size=200):",
                 "def dino_downsample(x, max_size=None):", "class UncertaintyModel(nn.Module):"):
        a = src.index(head)
        exec(src[a:src.index("\n\n\n", a)], ns)
    return ns


def run_reference(checkout, case, dtype, replay=None):
    """-> (outputs of the last step, dropout factors of every step, cache keys)."""
    rf = RecordingF()
    rf.replay = replay
    ns = reference_namespace(checkout, case, rf)
    config = types.SimpleNamespace(uncertainty_backbone="dinov2_vits14_reg", **L.CONFIG)
    model = ns["UncertaintyModel"](config)
    L.init_head(model, case)
    model = model.to(dtype)
    model.train(case["training"])
    torch.manual_seed(case["seed"])   # the reference draws its dropout mask from the global generator
    for step in range(case["steps"]):
        gt, pred = (t.to(dtype) for t in L.make_images(case, step))
        model.zero_grad()
        loss, metrics, loss_mult = model._compute_losses(gt, pred, prefix="", _cache_entry=f"image{step}")
    loss.backward()
    st = L.sample_stride(case)
    out = {"s": rf.softplus_out.detach()[0, 0], "loss_mult": loss_mult[0, 0],
           "result": torch.tensor([metrics[n] for n in L.RESULT_NAMES], dtype=torch.float64).to(dtype),
           "d_bn_weight": model.bn.weight.grad, "d_bn_bias": model.bn.bias.grad, "d_conv_weight": model.conv_seg.weight.grad.reshape(-1),
           "d_conv_bias": model.conv_seg.bias.grad, "running_mean": model.bn.running_mean, "running_var": model.bn.running_var}
    out = {k: v.detach().numpy().copy() for k, v in out.items()}
    assert loss_mult.shape == (1, 1, case["H"], case["W"]) and int(model.bn.num_batches_tracked) == 3 + (case["steps"] if case["training"] else 0)
    cache = sorted([k[0]] + list(k[1]) + list(v.shape) for k, v in model._images_cache.items())
    return out, rf.factors, cache, {n: float(metrics[n]) for n in L.RESULT_NAMES}, st


def main():
    checkout = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    torch.set_num_threads(1)
    arrays, meta, cases = {}, [], []
    for i, c in enumerate(L.CASES):
        o32, factors, cache, m32, st = run_reference(checkout, c, torch.float32)
        o64, factors64, cache64, m64, _ = run_reference(checkout, c, torch.float64, replay=factors)
        assert cache == cache64 and len(factors) == c["steps"]
        orc = L.run_oracle_case(c, factors)
        assert orc["clamp_margin"] >= 1e-5, (L.case_id(c), orc["clamp_margin"], "choose another seed")
        devs = {}
        for name in L.TENSORS:
            a, b = o32[name], o64[name]
            assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape, name
            devs[name] = float(np.abs(a.astype(np.float64) - b).max())
            if name == "loss_mult":
                a, b = a[::st, ::st], b[::st, ::st]
            arrays[f"c{i}_{name}32"], arrays[f"c{i}_{name}64"] = a, b
        arrays[f"c{i}_kdrop"] = np.stack(factors).astype(np.float64)
        meta.append({"ref32_dev": devs, "metrics32": m32, "metrics64": m64, "cache": cache, "clamp_margin": orc["clamp_margin"],
                     "frac_clip_min": orc["frac_clip_min"], "frac_clamp_max": orc["frac_clamp_max"]})
        cases.append(dict(c))
        print(f"{L.case_id(c):28s} loss {m64['loss']:.6f} margin {orc['clamp_margin']:.2e} at clip_min {orc['frac_clip_min']:.3f} at clamp_max "
              f"{orc['frac_clamp_max']:.3f} dino_part mean {orc['dino_part'].mean():.3f} (0: {np.mean(orc['dino_part'] == 0):.2f}, 1: "
              f"{np.mean(orc['dino_part'] == 1):.2f})  oracle-vs-ref64 " + " ".join(f"{n} {np.abs(orc[n] - o64[n]).max():.1e}" for n in L.TENSORS if n != "result")
              + f" result {np.abs(orc['result'][:7] - o64['result']).max():.1e}")
        print("    ref32_dev " + " ".join(f"{n} {d:.1e}" for n, d in devs.items()))
    np.savez_compressed(L.GOLDEN, cases=np.array(json.dumps(cases)), meta=np.array(json.dumps(meta)), **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
