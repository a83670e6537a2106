#!/usr/bin/env python3
"""Writes tests/golden/appearance_mlp_ref.npz: what the REFERENCE's own EmbeddingModel (wildgaussians/method.py:874-900) returns on the
cases of tests/appearance_mlp_lib.GOLDEN_CASES, on the CPU.

    python tests/golden/make_appearance_mlp_golden.py /path/to/reference/checkout

Runs only where a checkout of the reference lies.  As make_msssim_golden.py does for functions, the class body is executed out of method.py
(the module itself needs packages a test machine may lack).  The fixture holds recorded data only: per case the toned [P, 48] colours and
the gradients of sum(toned * cot) to the three inputs and the six parameters, in float32 and in float64.  Inputs, weights and cotangents
are regenerated from the seeds by tests/appearance_mlp_lib.
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import appearance_mlp_lib as L  # noqa: E402


def reference_class(checkout):
    src = open(os.path.join(checkout, "wildgaussians", "method.py")).read()
    ns = {"torch": torch, "nn": nn, "C0": L.C0, "Config": object}
    a = src.index("class EmbeddingModel(nn.Module):")
    exec(src[a:src.index("\n\n\n", a)], ns)  # the class body
    return ns["EmbeddingModel"]


def reference_model(cls, c, dtype):
    cfg = L.StubConfig(c["E"])
    cfg.appearance_n_fourier_freqs = c["G"] // 6   # the class sizes its first layer as E + 3 + 6 * n_fourier_freqs
    assert 6 * cfg.appearance_n_fourier_freqs == c["G"]
    return L.load_weights(cls(cfg), c["weights"], dtype)


def main():
    checkout = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    cls = reference_class(checkout)
    torch.set_num_threads(1)
    arrays = {}
    for i, (P, G, E, seed) in enumerate(L.GOLDEN_CASES):
        c = L.make_case(P, G, E, seed)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            res = L.run_module(cls.forward, reference_model(cls, c, dtype), c, True, dtype)
            for k, v in res.items():
                assert v.dtype == (np.float32 if tag == "32" else np.float64)
                arrays[f"{k}{tag}_{i}"] = v
        print(f"P {P} G {G} E {E} seed {seed}: discarded {c['discarded']:.3f}")
    np.savez_compressed(L.GOLDEN, cases=np.array(json.dumps(L.GOLDEN_CASES)), **arrays)
    print(L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
