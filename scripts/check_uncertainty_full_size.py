"""At the benchmark's two shapes: the fused operators and scripts/bench_uncertainty_step.py's float32 PyTorch restatement, each against the float64
oracle of tests/uncertainty_lib.py on the same features, dropout factors and metric maps: max |difference| per tensor.  Needs a HIP device."""
import os, sys, torch, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("wild-gaussians_amd", "tests", "scripts"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch.nn.functional as F
import uncertainty_lib as L, wg_fused_ssim as S, wg_fused_uncertainty as U, bench_uncertainty_step as B
dev = torch.device("cuda", 0)
for H, W in ((1200, 1600), (1080, 1920)):
    c = {"name": "big", "H": H, "W": W, "C": 384, "training": True, "init": "clamp", "steps": 1, "seed": H + W}
    gt, pred = L.make_images(c)
    model = L.StandInModel(c).to(dev)
    torch.manual_seed(1)
    kd = F.dropout2d(torch.ones(1, 384, 1, 1), 0.5, True).reshape(-1)
    feats = L.oracle_features(model.backbone, model.img_norm_mean.cpu(), model.img_norm_std.cpu(), gt, pred)
    gtd, predd = gt.to(dev), pred.to(dev)
    ss, ms = S.ssim_down(gtd, predd, max_size=400)[0], S.msssim(gtd, predd, max_size=400, min_size=80)[0]
    head = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in L.head_state(model).items()}
    ref = L.oracle(head, L.CONFIG, True, gt.double(), pred.double(), kd.double(), feats, ss.cpu(), ms.cpu())
    g = U.Geometry(H, W, 14)
    rm, rv = model.bn.running_mean.clone(), model.bn.running_var.clone()
    s = U.uncertainty_head(feats[0][0].to(dev), model.bn.weight, model.bn.bias, model.conv_seg.weight, model.conv_seg.bias, rm, rv, kd.to(dev), model.bn.eps, model.bn.momentum, True)
    loss, result, lm = U.uncertainty_loss(s, gtd, predd, ss, ms, feats[1][0].to(dev), feats[2][0].to(dev), g, 0.1, 0.5)
    loss.backward()
    d = lambda a, b: float(np.abs(a.detach().cpu().numpy().astype(np.float64) - b).max())
    print(H, W, "FUSED  s", d(s, ref["s"]), "loss_mult", d(lm[0, 0], ref["loss_mult"]), "result", d(result, ref["result"]),
          "dW", d(model.conv_seg.weight.grad.reshape(-1), ref["d_conv_weight"]), "margin", ref["clamp_margin"], flush=True)
    # the bench's restatement with the same features and mask
    m2 = B.PrecomputedModel(c).to(dev)
    m2.pre = {}
    shapes = [(1, 3, g.Hp, g.Wp), (1, 3, g.nhp, g.nwp), (1, 3, g.nhp, g.nwp)]
    for (shape, named, f) in zip(shapes, (True, True, False), feats):
        m2.pre[(shape, named)] = f.to(dev)
    orig = F.dropout2d
    F.dropout2d = lambda x, p=0.5, training=True, inplace=False: x * kd.to(dev).reshape(1, -1, 1, 1)
    try:
        l2, met, lm2 = B.torch_compute_losses(m2, gtd, predd, "", _cache_entry="k")
        l2.backward()
    finally:
        F.dropout2d = orig
    r2 = np.array([met[n] for n in L.RESULT_NAMES])
    print(H, W, "TORCH  loss_mult", d(lm2[0, 0], ref["loss_mult"]), "result", float(np.abs(r2 - ref["result"][:7]).max()),
          "dW", d(m2.conv_seg.weight.grad.reshape(-1), ref["d_conv_weight"]), "ref loss", ref["result"][0], flush=True)
