"""Shared by tests/test_appearance_colour.py, tests/golden/make_appearance_colour_golden.py and scripts/bench_appearance_colour.py: seeded
inputs with robust rows, and the float64 oracle of the toned-colour operator (include/wg_appearance_colour.h; wildgaussians/method.py:1555,
:1557, :890-900, :1592-1598) that carries, beside every value, an A-PRIORI float32 rounding bound.

The MLP's values and bounds are appearance_mlp_lib's (`mm`, `forward64`, `backward64`).  Around it, every float32 operation rounds once
(relative error u = 2^-24; a fused multiply-add rounds once where the two separate operations round twice, and the bound of the two covers
it), constants are their float32 roundings (u each), and the bounds hold for ANY order of evaluation:

    product of m factors f_i known to within e_i    |computed - prod f_i| <= prod (|f_i| + e_i) (1 + u)^(m - 1) - prod |f_i|
    sum of n terms t_i known to within e_i          |computed - sum t_i|  <= sum e_i + gamma(n - 1) sum (|t_i| + e_i)

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a term passes through at most n - 1 additions.)  The direction
d = v / max(|v|, 1e-12), v = xyz - campos: v rounds once; v_i^2 carries 3 factors (1 + delta); the sum of three squares 2 more; the square
root halves the 5 and rounds once (at most 4 factors); the division v_i / |v| carries 1 + 4 + 1 = 6, so |d_i computed - d_i| <= gamma(6) |d_i|.
Each basis polynomial Y_k(d) is built from the two rules above, operation for operation as eval_sh writes it.  A clamp or a ReLU is exact
where its decision is the float64 one; `robust` keeps only rows on which no float32 evaluation within the bounds can flip a decision: the
ReLU masks (appearance_mlp_lib.robust_rows), every t against post_clamp_max, and 0.5 + sum against 0 at every degree.  Sums over rows use
gamma(n) with n the number of listed rows whose cotangent is non-zero (backward64).  Nothing here is tuned to any implementation."""
import math
import os

import numpy as np
import torch

import appearance_mlp_lib as ML
from appearance_mlp_lib import MAX_DISCARD, backward64, forward64, gamma, mm, ratio, robust_rows  # noqa: F401  (mm: the MLP's product rule)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "appearance_colour_ref.npz")
U, C0, OUT_SCALE = ML.U, ML.C0, ML.OUT_SCALE
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
CAMPOS = (0.3, -0.2, 4.5)
NCOEF = 16


# ---- (value, bound) arithmetic ------------------------------------------------------------------------------------------------------------
def const(c):
    """A double constant as a float32 evaluation holds it."""
    return (c, abs(c) * U)


def exact(v):
    return (v, torch.zeros_like(v) if torch.is_tensor(v) else 0.0)


def _abs(v):
    return v.abs() if torch.is_tensor(v) else abs(v)


def prod(*fs):
    val, hi, lo = 1.0, 1.0, 1.0
    for f, e in fs:
        val, hi, lo = val * f, hi * (_abs(f) + e), lo * _abs(f)
    return val, hi * (1 + U) ** (len(fs) - 1) - lo


def ssum(*ts):
    val = sum(t for t, _ in ts)
    err = sum(e for _, e in ts)
    mag = sum(_abs(t) + e for t, e in ts)
    return val, err + gamma(len(ts) - 1) * mag


def neg(a):
    return (-a[0], a[1])


def direction64(xyz, campos):
    """-> three (value, bound) pairs, the components of normalize(xyz - campos)."""
    v = xyz.double() - campos.double()
    d = v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return [(d[:, i], gamma(6) * d[:, i].abs()) for i in range(3)]


def basis64(x, y, z):
    """The 16 polynomials of eval_sh (method.py:510-536) as (value, bound) pairs at the direction (x, y, z), each itself a pair."""
    two, three, four = exact(2.0), exact(3.0), exact(4.0)
    xx, yy, zz, xy, yz, xz = prod(x, x), prod(y, y), prod(z, z), prod(x, y), prod(y, z), prod(x, z)
    one = torch.ones_like(x[0])
    Y = [(C0 * one, U * C0 * one)]
    Y += [prod(const(-C1), y), prod(const(C1), z), prod(const(-C1), x)]
    Y += [prod(const(C2[0]), xy), prod(const(C2[1]), yz), prod(const(C2[2]), ssum(prod(two, zz), neg(xx), neg(yy))), prod(const(C2[3]), xz),
          prod(const(C2[4]), ssum(xx, neg(yy)))]
    Y += [prod(const(C3[0]), y, ssum(prod(three, xx), neg(yy))),
          prod(const(C3[1]), xy, z),
          prod(const(C3[2]), y, ssum(prod(four, zz), neg(xx), neg(yy))),
          prod(const(C3[3]), z, ssum(prod(two, zz), neg(prod(three, xx)), neg(prod(three, yy)))),
          prod(const(C3[4]), x, ssum(prod(four, zz), neg(xx), neg(yy))),
          prod(const(C3[5]), z, ssum(xx, neg(yy))),
          prod(const(C3[6]), x, ssum(xx, neg(prod(three, yy))))]
    return Y


# ---- the operator --------------------------------------------------------------------------------------------------------------------------
def colour_forward64(features, gemb, emb, xyz, campos, W, pre=1.0, post=1.0, scale=OUT_SCALE):
    """Everything up to the SH sum, float64 with bounds, for all rows.  W: the six float64 weights.  -> dict."""
    P = features.shape[0]
    fc = features.double().clamp_max(pre)[:, :3 * NCOEF]
    x = torch.cat([fc[:, :3], gemb.double(), emb.double()[None].repeat(P, 1)], 1)
    f = forward64(x, W, scale=scale)
    t, e_t = ML.tone64(fc, f["out"], f["e_out"])
    keep = t <= post                                   # the clamp passes the value (and the cotangent) through
    tc, e_tc = torch.where(keep, t, torch.full_like(t, post)), e_t * keep
    Y = basis64(*direction64(xyz, campos))
    return dict(x=x, f=f, fc=fc, t=t, e_t=e_t, keep=keep, tc=tc, e_tc=e_tc, Y=Y, post=post)


def colour_sum64(s, deg):
    """-> (0.5 + sum_k Y_k t_k [P, 3], its bound)."""
    n = (deg + 1) ** 2
    val, err = [], []
    for c in range(3):
        terms = [prod(s["Y"][k], (s["tc"][:, 3 * k + c], s["e_tc"][:, 3 * k + c])) for k in range(n)]
        v, e = ssum(exact(torch.full_like(terms[0][0], 0.5)), *terms)
        val.append(v)
        err.append(e)
    return torch.stack(val, 1), torch.stack(err, 1)


def robust(features, gemb, emb, xyz, campos, W, pre=1.0, post=1.0):
    """Mask of the rows on which no decision can flip within twice its bound, and the share lost to each kind of decision."""
    s = colour_forward64(features, gemb, emb, xyz, campos, W, pre, post)
    relu = robust_rows(s["x"], W)
    clamp = torch.ones_like(relu) if math.isinf(post) else ((s["t"] - post).abs() > 2 * s["e_t"]).all(1)
    floor = torch.ones_like(relu)
    for deg in range(4):
        v, e = colour_sum64(s, deg)
        floor &= (v.abs() > 2 * e).all(1)
    return relu & clamp & floor, dict(relu=1 - float(relu.double().mean()), clamp=1 - float(clamp.double().mean()),
                                      floor=1 - float(floor.double().mean()))


def draw_weights(K, seed):
    """appearance_mlp_lib.draw_weights with b3[0:3] in U[-20, 20] and b3[3:6] in U[50, 150]: offset within +-0.2 and mul near 1 (the
    reference's untrained mul is near 0.003 and would leave every clamp idle)."""
    W = ML.draw_weights(K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    W[5] = torch.cat([torch.rand(3, generator=g) * 40 - 20, torch.rand(3, generator=g) * 100 + 50]).float()
    return W


def make_case(P, G, E, seed, pre=1.0, post=1.0):
    """-> dict of float32 CPU tensors: features [P, 48] in U[-0.25, 1.5], gemb [P, G] in U[-1, 1], emb [E] ~ N(0, 0.3^2), xyz [P, 3] ~
    N(0, 2^2), campos [3], weights, and `discarded`, the share of the 2 P candidate rows that were not robust (`lost`: per decision).  The
    first P robust candidates are kept."""
    g = torch.Generator().manual_seed(seed)
    K = 3 + G + E
    W = draw_weights(K, seed + 7919)
    n = 2 * P
    feats = torch.rand(n, 3 * NCOEF, generator=g) * 1.75 - 0.25
    gemb = torch.rand(n, G, generator=g) * 2 - 1
    emb = torch.randn(E, generator=g) * 0.3
    xyz = torch.randn(n, 3, generator=g) * 2
    campos = torch.tensor(CAMPOS)
    ok, lost = robust(feats, gemb, emb, xyz, campos, [w.double() for w in W], pre, post)
    keep = ok.nonzero()[:P, 0]
    assert len(keep) == P, f"only {len(keep)} robust rows among {n} candidates"
    return dict(P=P, G=G, E=E, K=K, seed=seed, features=feats[keep].contiguous(), gemb=gemb[keep].contiguous(), emb=emb,
                xyz=xyz[keep].contiguous(), campos=campos, weights=W, pre=pre, post=post, discarded=1.0 - float(ok.double().mean()), lost=lost)


def dense_cotangent(P, seed):
    return torch.randn(P, 3, generator=torch.Generator().manual_seed(seed + 31))


def sparse_cotangent(P, seed, block=64):
    """Non-zero on one row of every `block`-row block (a different offset per block), plus the first and the last row."""
    return ML.sparse_cotangent(P, seed, block)[:, :3].contiguous()


def scattered_rows(P, M, seed):
    """M distinct rows of P, unsorted."""
    return torch.randperm(P, generator=torch.Generator().manual_seed(seed + 77))[:M]


def oracle(c, cot, deg, rows=None, scale=OUT_SCALE):
    """Float64 values and bounds for case c: `colours` [P, 3] (zero with a zero bound on rows not listed) and, for the cotangent cot [P, 3]
    (read on listed rows only), `grad` [E].  Also the shares of active decisions, for the tests that want every branch exercised."""
    W = [w.double() for w in c["weights"]]
    P = c["P"]
    idx = torch.arange(P) if rows is None else rows.long()
    s = colour_forward64(c["features"][idx], c["gemb"][idx], c["emb"], c["xyz"][idx], c["campos"], W, c["pre"], c["post"], scale=scale)
    n = (deg + 1) ** 2
    v, e = colour_sum64(s, deg)
    on = v > 0
    colours, e_colours = torch.zeros(P, 3, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64)
    colours[idx], e_colours[idx] = v * on, e * on
    g = cot.double()[idx] * on
    doff, dmul = [], []
    for ch in range(3):
        gc = exact(g[:, ch])
        terms = []
        for k in range(n):
            m = s["keep"][:, 3 * k + ch]
            dt = prod(s["Y"][k], gc)
            dt = (dt[0] * m, dt[1] * m)
            terms.append(prod(dt, exact(s["fc"][:, 3 * k + ch])))
            if k == 0:
                q = dt[0] / C0
                doff.append((q, dt[1] / C0 + 2 * U * (q.abs() + dt[1] / C0)))   # the divisor rounded to float32, and the division
        dmul.append(ssum(*terms) if len(terms) > 1 else terms[0])
    dom = torch.stack([p[0] for p in doff + dmul], 1)
    e_dom = torch.stack([p[1] for p in doff + dmul], 1)
    r = backward64(s["x"], W, s["f"], dom, ecot=e_dom, n_shared=c["E"])
    used = s["keep"].view(-1, NCOEF, 3)[:, :n]
    return dict(colours=colours, e_colours=e_colours, grad=r["dshared"], e_grad=r["e_dshared"], om=s["f"]["out"],
                clamped=1 - float(used.double().mean()), floored=1 - float(on.double().mean()))


# ---- the reference's own statements, for the fixture ----------------------------------------------------------------------------------------
GOLDEN_CASES = [(1, 24, 32, 21, 3), (65, 24, 32, 22, 3), (37, 6, 5, 24, 2)]   # (P, G, E, seed, deg)


def golden_cot(P, seed):
    return torch.randn(P, 3, generator=torch.Generator().manual_seed(seed + 101))


def run_reference(model, eval_sh, c, deg, dtype):
    """The caller's inline statements (method.py:1555, :1557, :1587, :1592-1598) around the reference's EmbeddingModel and eval_sh, on case c
    in `dtype` -> (colours [P, 3], d embedding [E]) as numpy arrays, for the cotangent golden_cot."""
    F = torch.nn.functional
    features = c["features"].to(dtype).clamp_max(1.0)
    means3D, camera_center = c["xyz"].to(dtype), c["campos"].to(dtype)
    embedding = c["emb"].to(dtype).clone().requires_grad_(True)
    dir_pp_normalized = F.normalize(means3D - camera_center.repeat(features.shape[0], 1), dim=1)
    embedding_expanded = embedding[None].repeat(len(means3D), 1)
    colors_toned = model(c["gemb"].to(dtype), embedding_expanded, features).clamp_max(1.0)
    shdim = 16
    colors_toned = colors_toned.view(-1, shdim, 3).transpose(1, 2).contiguous().clamp_max(1.0)
    colors_toned = eval_sh(deg, colors_toned, dir_pp_normalized)
    colors_toned = torch.clamp_min(colors_toned + 0.5, 0.0)
    (colors_toned * golden_cot(c["P"], c["seed"]).to(dtype)).sum().backward()
    return colors_toned.detach().numpy(), embedding.grad.numpy()


# ---- the same colours by other means: plain PyTorch, and the chain of the project's existing operators ----------------------------------------
def sh_sum_torch(deg, sh, d):
    """sum_k Y_k(d) sh[..., k] for sh [P, 3, 16] and unit directions d [P, 3], in sh's dtype: the polynomials of `basis64` as tensor operations."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    out = C0 * sh[..., 0]
    if deg > 0:
        out = out - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out = (out + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6] + C2[3] * xz * sh[..., 7]
               + C2[4] * (xx - yy) * sh[..., 8])
    if deg > 2:
        out = (out + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10] + C3[2] * y * (4 * zz - xx - yy) * sh[..., 11]
               + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12] + C3[4] * x * (4 * zz - xx - yy) * sh[..., 13]
               + C3[5] * z * (xx - yy) * sh[..., 14] + C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return out


def _tone(fc, om, post):
    offset, mul = om[:, :3], om[:, 3:]
    offset = torch.cat((offset / C0, torch.zeros_like(fc[:, 3:])), dim=-1)
    toned = (fc * mul.repeat(1, fc.shape[1] // 3) + offset).clamp_max(post)
    return toned.view(-1, NCOEF, 3).transpose(1, 2).contiguous().clamp_max(post)


def torch_chain(features, gemb, emb, xyz, campos, W, deg, pre=1.0, post=1.0):
    """The caller's chain in plain PyTorch, every intermediate tensor materialised, in the inputs' dtype."""
    fc = features[:, :3 * NCOEF].clamp_max(pre)
    d = torch.nn.functional.normalize(xyz - campos.repeat(fc.shape[0], 1), dim=1)
    x = torch.cat((fc[:, :3], gemb, emb[None].repeat(fc.shape[0], 1)), dim=-1)
    om = (torch.relu(torch.relu(x @ W[0].t() + W[1]) @ W[2].t() + W[3]) @ W[4].t() + W[5]) * 0.01
    return torch.clamp_min(sh_sum_torch(deg, _tone(fc, om, post), d) + 0.5, 0.0)


def operator_chain(FG, features, gemb, emb, xyz, campos, W, deg, pre=1.0, post=1.0, max_workgroups=0):
    """The chain of the project's existing opt-in operators: appearance_mlp(shared=), the tone in PyTorch, wg_fused_gaussians.eval_sh."""
    fc = features[:, :3 * NCOEF].clamp_max(pre)
    d = torch.nn.functional.normalize(xyz - campos.repeat(fc.shape[0], 1), dim=1)
    om = FG.appearance_mlp((fc[:, :3], gemb), W, shared=emb, max_workgroups=max_workgroups)
    return torch.clamp_min(FG.eval_sh(deg, _tone(fc, om, post), d) + 0.5, 0.0)
