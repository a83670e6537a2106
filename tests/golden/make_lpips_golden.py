#!/usr/bin/env python3
"""Writes tests/golden/lpips_ref.npz: what the REFERENCE's own `LPIPS` class (wildgaussians/_metrics_lpips.py) returns on the cases of
tests/lpips_lib.py, on the CPU, in float32 and in float64, fed as `evaluation._lpips` feeds it (clip to [0, 1], * 2, - 1).

    python tests/golden/make_lpips_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies: _metrics_lpips.py is imported by its path.  It imports `torchvision.models` for the trunks'
layer lists only; where torchvision is not installed, a stand-in module of that name is registered whose `alexnet()` / `vgg16()` return an
object with the standard `.features` nn.Sequential (tests/lpips_lib.feature_layers).  The model is built as
`LPIPS(net, pretrained=False, pnet_rand=True, verbose=False)` -- nothing is downloaded -- and tests/lpips_lib.make_weights() is loaded into it
strictly: every name of the state dict is generated.

The fixture holds recorded data only.  Per case: the float64 total and five layer values [B] / [B, 5] and the float32 run's deviations from
them; per tap, every 16th channel of the float64 features of the FIRST argument's images (hooked from the reference's trunk), and over the
whole tap tensors of both arguments ref32_dev = max |float32 - float64| and max_abs.  Inputs and weights are regenerated from seeds.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_lib as L  # noqa: E402


def reference_module(checkout):
    try:
        import torchvision.models  # noqa: F401
    except ImportError:
        tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
        models.alexnet = lambda pretrained=False, **kw: types.SimpleNamespace(features=L.feature_layers("alex"))
        models.vgg16 = lambda pretrained=False, **kw: types.SimpleNamespace(features=L.feature_layers("vgg"))
        tv.models = models
        sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    spec = importlib.util.spec_from_file_location("wg_reference_metrics_lpips", os.path.join(checkout, "wildgaussians", "_metrics_lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, c, dtype):
    """-> (total [B], layers [B, 5], taps of the first argument, taps of the second), as float64 arrays computed in `dtype`."""
    model = mod.LPIPS(net=c["net"], pretrained=False, pnet_rand=True, verbose=False)
    model.load_state_dict(L.make_weights(c["net"]), strict=True)
    model = model.to(dtype).eval()
    seen = []   # the reference calls its trunk's `forward` directly, so the hooks sit on the five slices: first argument's pass, then the second's
    handles = [getattr(model.net, f"slice{s + 1}").register_forward_hook(lambda m, args, out: seen.append(out.detach().double().numpy().copy()))
               for s in range(L.TAPS)]
    pred, gt = L.make_images(c)
    feed = lambda x: x.clamp(0, 1).to(dtype).mul_(2).sub_(1)      # float32 operations in the float32 run, exact in the float64 one
    with torch.no_grad():
        val, res = model.forward(feed(pred), feed(gt), retPerLayer=True)
    for handle in handles:
        handle.remove()
    assert len(seen) == 2 * L.TAPS
    layers = torch.cat([r.reshape(c["B"], 1) for r in res], dim=1)
    return val.reshape(c["B"]).double().numpy(), layers.double().numpy(), seen[:L.TAPS], seen[L.TAPS:]


def main(checkout):
    torch.manual_seed(0)
    mod = reference_module(checkout)
    arrays = {}
    for c in L.CASES:
        v32, l32, a32, b32 = run_reference(mod, c, torch.float32)
        v64, l64, a64, b64 = run_reference(mod, c, torch.float64)
        n = c["name"]
        arrays[n + "/total64"], arrays[n + "/layers64"] = v64, l64
        arrays[n + "/total32_dev"], arrays[n + "/layers32_dev"] = np.abs(v32 - v64), np.abs(l32 - l64)
        for l in range(L.TAPS):
            arrays[f"{n}/tap{l}_64"] = np.ascontiguousarray(a64[l][:, ::L.CHANNEL_STRIDE])
            arrays[f"{n}/tap{l}_ref32_dev"] = np.float64(max(np.abs(a32[l] - a64[l]).max(), np.abs(b32[l] - b64[l]).max()))
            arrays[f"{n}/tap{l}_max_abs"] = np.float64(max(np.abs(a64[l]).max(), np.abs(b64[l]).max()))
        total, layers, t0, t1 = L.run_oracle_case(n)
        worst = max(max(np.abs(x - y).max() for x, y in zip(t0, a64)), max(np.abs(x - y).max() for x, y in zip(t1, b64)))
        print(f"{n}: total {v64.round(4)}, float32 deviation {np.abs(v32 - v64).max():.2e}; layers {l64[0].round(4)}; tap ref32_dev "
              f"{[float('%.1e' % arrays[f'{n}/tap{l}_ref32_dev']) for l in range(L.TAPS)]}, max_abs {[round(float(arrays[f'{n}/tap{l}_max_abs']), 2) for l in range(L.TAPS)]}; "
              f"max|oracle - reference float64|: taps {worst:.1e}, values {max(np.abs(total - v64).max(), np.abs(layers - l64).max()):.1e}")
    np.savez_compressed(L.GOLDEN, **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")
    assert os.path.getsize(L.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main(sys.argv[1])
