"""Shared by tests/test_appearance_mlp.py and tests/golden/make_appearance_mlp_golden.py: seeded inputs with robust rows, and the float64
oracle of the appearance MLP (wildgaussians/method.py:890-897) that carries, beside every value, an A-PRIORI float32 rounding bound.

The bound holds for ANY summation order of a float32 evaluation with one rounding per operation (fmaf chains included).  For a product
C = A . B over n terms whose inputs are known to within eA, eB (elementwise):

    eC = eA |B| + |A| eB + eA eB + gamma(n + 1) (|A| + eA)(|B| + eB),     gamma(n) = n u / (1 - n u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: each term passes through at most n roundings -- its product and at
most n - 1 additions; the bias is one more term).  out_scale is float32(0.01) and costs one rounding.  Sums over rows use gamma(n) with
n the number of rows whose cotangent is non-zero: a zero cotangent gives exact zeros in every backward product, and adding an exact zero
does not round.  ReLU masks are taken from the float64 values; `robust_rows` keeps only rows on which no float32 evaluation within the
bound can flip one.  Nothing here is tuned to any implementation."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "appearance_mlp_ref.npz")
U = 2.0 ** -24
C0 = 0.28209479177387814
OUT_SCALE = float(np.float32(0.01))
HID, NOUT = 128, 6
MAX_DISCARD = 0.10


def gamma(n):
    return n * U / (1 - n * U)


def mm(A, eA, B, eB, n, extra=None):
    """A . B with its bound; `extra` (the bias) joins the magnitude as one more term (n + 1 roundings at most either way)."""
    C = A @ B
    mag = (A.abs() + eA) @ (B.abs() + eB)
    if extra is not None:
        mag = mag + extra.abs()
    return C, eA @ B.abs() + A.abs() @ eB + eA @ eB + gamma(n + 1) * mag


def draw_weights(K, seed):
    """nn.Linear's default range, U(+-1/sqrt(fan_in)), float32: W1 [128, K] b1 W2 [128, 128] b2 W3 [6, 128] b3."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(HID, K), (HID,), (HID, HID), (HID,), (NOUT, HID), (NOUT,)]
    fan = [K, K, HID, HID, HID, HID]
    return [((torch.rand(s, generator=g) * 2 - 1) / math.sqrt(f)).float() for s, f in zip(shapes, fan)]


def forward64(x, W, scale=OUT_SCALE):
    """x [P, K] float64, W the six float64 weights -> dict of values and bounds.  scale: float32(0.01), what a float32 evaluation
    multiplies by; with the double 0.01 instead (what the reference's own float64 run multiplies by, so what the fixture records) the
    bound also covers the constant's conversion to float32, |float32(0.01) - 0.01| / 0.01 = 0.37 u."""
    conv = abs(OUT_SCALE - scale) / scale
    z0 = torch.zeros_like(x)
    K = x.shape[1]
    z1, e1 = mm(x, z0, W[0].t(), torch.zeros_like(W[0].t()), K, W[1])
    z1 = z1 + W[1]
    m1 = z1 > 0
    h1, eh1 = z1 * m1, e1 * m1
    z2, e2 = mm(h1, eh1, W[2].t(), torch.zeros_like(W[2].t()), HID, W[3])
    z2 = z2 + W[3]
    m2 = z2 > 0
    h2, eh2 = z2 * m2, e2 * m2
    z3, e3 = mm(h2, eh2, W[4].t(), torch.zeros_like(W[4].t()), HID, W[5])
    z3 = z3 + W[5]
    out = z3 * scale
    eo = e3 * scale + (U + conv) * (out.abs() + e3 * scale)
    return dict(scale=scale, conv=conv, z1=z1, e1=e1, m1=m1, h1=h1, eh1=eh1, z2=z2, e2=e2, m2=m2, h2=h2, eh2=eh2, out=out, e_out=eo)


def backward64(x, W, f, cot, ecot=None, n_shared=0):
    """Gradients of sum(out * cot) with bounds.  `cot` [P, 6] float64, known to within `ecot`.  n_shared: the last n_shared columns of x
    are one vector repeated; `dshared` is then the row sum of their gradient, bounded as a sum of n * 128 products in any nesting."""
    P = x.shape[0]
    ecot = torch.zeros_like(cot) if ecot is None else ecot
    n = max(int(((cot != 0) | (ecot != 0)).any(1).sum()), 1)
    scale, conv = f["scale"], f["conv"]
    dz3 = cot * scale
    edz3 = ecot * scale + (U + conv) * (dz3.abs() + ecot * scale)
    zW = [torch.zeros_like(w) for w in W]
    r = {}
    r["dW3"], r["e_dW3"] = mm(dz3.t(), edz3.t(), f["h2"], f["eh2"], n)
    r["db3"], r["e_db3"] = dz3.sum(0), edz3.sum(0) + gamma(n) * (dz3.abs() + edz3).sum(0)
    dh2, edh2 = mm(dz3, edz3, W[4], zW[4], NOUT)
    dz2, edz2 = dh2 * f["m2"], edh2 * f["m2"]
    r["dW2"], r["e_dW2"] = mm(dz2.t(), edz2.t(), f["h1"], f["eh1"], n)
    r["db2"], r["e_db2"] = dz2.sum(0), edz2.sum(0) + gamma(n) * (dz2.abs() + edz2).sum(0)
    dh1, edh1 = mm(dz2, edz2, W[2], zW[2], HID)
    dz1, edz1 = dh1 * f["m1"], edh1 * f["m1"]
    r["dW1"], r["e_dW1"] = mm(dz1.t(), edz1.t(), x, torch.zeros_like(x), n)
    r["db1"], r["e_db1"] = dz1.sum(0), edz1.sum(0) + gamma(n) * (dz1.abs() + edz1).sum(0)
    r["dx"], r["e_dx"] = mm(dz1, edz1, W[0], zW[0], HID)
    if n_shared:
        Ws = W[0][:, -n_shared:].abs()
        r["dshared"] = r["dx"][:, -n_shared:].sum(0)
        # sum over rows and over the 128 units, in either nesting: at most n + 128 roundings on any term's path
        r["e_dshared"] = (edz1 @ Ws).sum(0) + gamma(n + HID + 1) * ((dz1.abs() + edz1) @ Ws).sum(0)
    return r


def robust_rows(x, W):
    """Mask of the rows of x (float64) on which every |z1| and |z2| exceeds twice its bound."""
    f = forward64(x, W)
    return (f["z1"].abs() > 2 * f["e1"]).all(1) & (f["z2"].abs() > 2 * f["e2"]).all(1)


def make_case(P, G, E, seed, colour_width=48):
    """-> dict of float32 CPU tensors: features [P, colour_width] in U[0, 1] (colour = its first 3 columns), gemb [P, G] in U[-1, 1],
    aemb_row [E] ~ N(0, 0.3^2) (the shared vector; the per-row form is its repeat, as the reference's caller builds it), weights, and
    `discarded`, the fraction of the 2 P candidate rows that were not robust.  The first P robust candidates are kept."""
    g = torch.Generator().manual_seed(seed)
    K = 3 + G + E
    W = draw_weights(K, seed + 7919)
    n = 2 * P
    feats = torch.rand(n, colour_width, generator=g)
    gemb = torch.rand(n, G, generator=g) * 2 - 1
    aemb = torch.randn(E, generator=g) * 0.3
    x = torch.cat([feats[:, :3], gemb, aemb[None].repeat(n, 1)], 1).double()
    ok = robust_rows(x, [w.double() for w in W])
    keep = ok.nonzero()[:P, 0]
    assert len(keep) == P, f"only {len(keep)} robust rows among {n} candidates"
    return dict(P=P, G=G, E=E, K=K, seed=seed, features=feats[keep].contiguous(), gemb=gemb[keep].contiguous(), aemb=aemb, weights=W,
                discarded=1.0 - float(ok.double().mean()))


def case_x64(c):
    return torch.cat([c["features"][:, :3], c["gemb"], c["aemb"][None].repeat(c["P"], 1)], 1).double()


def dense_cotangent(P, seed):
    return torch.randn(P, NOUT, generator=torch.Generator().manual_seed(seed + 31))


def sparse_cotangent(P, seed, block=64):
    """Non-zero on one row of every `block`-row block (a different offset per block), plus the first and the last row."""
    g = torch.Generator().manual_seed(seed + 57)
    cot = torch.zeros(P, NOUT)
    rows = set([0, P - 1])
    for b in range((P + block - 1) // block):
        lo, hi = b * block, min(P, (b + 1) * block)
        rows.add(lo + int(torch.randint(0, hi - lo, (1,), generator=g)))
    rows = sorted(rows)
    cot[rows] = torch.randn(len(rows), NOUT, generator=g)
    return cot


def oracle(c, cot):
    """Everything the kernel tests compare against, for case c and cotangent cot [P, 6]."""
    x, W = case_x64(c), [w.double() for w in c["weights"]]
    f = forward64(x, W)
    r = backward64(x, W, f, cot.double(), n_shared=c["E"])
    r["out"], r["e_out"] = f["out"], f["e_out"]
    return r


def ratio(got, want, bound):
    """max |got - want| / bound over all elements (0 where both the error and the bound are 0)."""
    err = (got.detach().double().cpu() - want).abs()
    if err.numel() == 0:
        return 0.0
    q = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(q.max())


# ---- the module's tail: the two torch statements after the MLP (method.py:898-900), in float64 with bounds -------------------------------
def tone64(features, om, e_om):
    """input_color * mul.repeat + cat(offset / C0, 0) for om = (offset, mul) [P, 6] known to within e_om.  The float32 evaluation rounds
    offset / C0 (the divisor itself rounded to float32: 2 u), the product and the sum (u each)."""
    c = features.double()
    rep = c.shape[1] // 3
    off, e_off = om[:, :3] / C0, e_om[:, :3] / C0
    e_off = e_off + 2 * U * (off.abs() + e_off)
    mul, e_mul = om[:, 3:].repeat(1, rep), e_om[:, 3:].repeat(1, rep)
    offp = torch.cat([off, torch.zeros_like(c[:, 3:])], 1)
    e_offp = torch.cat([e_off, torch.zeros_like(c[:, 3:])], 1)
    prod = c * mul
    val = prod + offp
    e = c.abs() * e_mul + e_offp
    e = e + U * (prod.abs() + c.abs() * e_mul) + U * (val.abs() + e) * (1 + U)
    return val, e


def tone_backward64(features, om, e_om, cot48):
    """-> (d om [P, 6], its bound, d features through the tail alone [P, 48], its bound) for the cotangent cot48 [P, 48] of the toned
    colours.  d mul[p, j] sums 16 products (the repeat's backward); d offset = cot / C0."""
    c, ct = features.double(), cot48.double()
    P, Cw = c.shape
    rep = Cw // 3
    prod = (ct * c).view(P, rep, 3)
    dmul = prod.sum(1)
    e_dmul = gamma(rep + 1) * prod.abs().sum(1)
    doff = ct[:, :3] / C0
    e_doff = 2 * U * doff.abs()
    mul, e_mul = om[:, 3:].repeat(1, rep), e_om[:, 3:].repeat(1, rep)
    dfeat = ct * mul
    e_dfeat = ct.abs() * e_mul + U * (dfeat.abs() + ct.abs() * e_mul)
    return torch.cat([doff, dmul], 1), torch.cat([e_doff, e_dmul], 1), dfeat, e_dfeat


def module_oracle(c, cot48):
    """EmbeddingModel.forward and the gradients of sum(result * cot48), float64 with bounds: keys toned, d_features, d_gemb, d_aemb_rows
    [P, E], dshared [E], dW1..db3, each with its e_ twin."""
    x, W = case_x64(c), [w.double() for w in c["weights"]]
    f = forward64(x, W, scale=0.01)   # the fixture's float64 arrays were computed with the double constant
    toned, e_toned = tone64(c["features"], f["out"], f["e_out"])
    dom, e_dom, dfeat, e_dfeat = tone_backward64(c["features"], f["out"], f["e_out"], cot48)
    r = backward64(x, W, f, dom, ecot=e_dom, n_shared=c["E"])
    G = c["G"]
    dfeat = dfeat.clone()
    e_dfeat = e_dfeat.clone()
    a, ea = r["dx"][:, :3], r["e_dx"][:, :3]
    s = dfeat[:, :3] + a
    e_dfeat[:, :3] = e_dfeat[:, :3] + ea + U * (s.abs() + e_dfeat[:, :3] + ea)   # autograd adds the two paths: one more rounding
    dfeat[:, :3] = s
    r.update(toned=toned, e_toned=e_toned, d_features=dfeat, e_d_features=e_dfeat, d_gemb=r["dx"][:, 3:3 + G], e_d_gemb=r["e_dx"][:, 3:3 + G],
             d_aemb_rows=r["dx"][:, 3 + G:], e_d_aemb_rows=r["e_dx"][:, 3 + G:])
    return r


# the fixture's cases: (P, G, E, seed)
GOLDEN_CASES = [(1, 24, 32, 11), (65, 24, 32, 12), (37, 6, 5, 14)]
GOLDEN_KEYS = ["toned", "d_features", "d_gemb", "d_aemb", "dW1", "db1", "dW2", "db2", "dW3", "db3"]


def golden_cot48(P, seed):
    return torch.randn(P, 48, generator=torch.Generator().manual_seed(seed + 101))


def run_module(forward, model, c, per_row, dtype, device="cpu"):
    """forward(model, gembedding, aembedding, color) on case c, with `model` holding c's weights in `dtype`, and the gradients of
    sum(result * cot48) -> dict of numpy arrays under GOLDEN_KEYS (d_aemb has the aembedding's shape: [P, E] per row, [E] shared)."""
    feats = c["features"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    gemb = c["gemb"].detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    a = c["aemb"].detach().clone().to(device=device, dtype=dtype)
    aemb = (a[None].repeat(c["P"], 1) if per_row else a.clone()).requires_grad_(True)
    cot = golden_cot48(c["P"], c["seed"]).to(device=device, dtype=dtype)
    for p in model.parameters():
        p.grad = None
    toned = forward(model, gemb, aemb, feats)
    (toned * cot).sum().backward()
    lin = [m for m in model.mlp if isinstance(m, torch.nn.Linear)]
    vals = [toned, feats.grad, gemb.grad, aemb.grad, lin[0].weight.grad, lin[0].bias.grad, lin[1].weight.grad, lin[1].bias.grad,
            lin[2].weight.grad, lin[2].bias.grad]
    return {k: v.detach().cpu().numpy() for k, v in zip(GOLDEN_KEYS, vals)}


class StubConfig:
    appearance_model_sh = False
    sh_degree = 3
    appearance_n_fourier_freqs = 4

    def __init__(self, E):
        self.appearance_embedding_dim = E


def load_weights(model, W, dtype, device="cpu"):
    lin = [m for m in model.mlp if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (w, b) in zip(lin, [(W[0], W[1]), (W[2], W[3]), (W[4], W[5])]):
            m.weight.copy_(w)
            m.bias.copy_(b)
    return model.to(device=device, dtype=dtype)


class StubEmbedding(torch.nn.Module):
    """What embedding_forward needs of an EmbeddingModel: `config.appearance_model_sh` and `mlp`.  Its own forward only records the call (it
    stands for the caller's code, which the uncovered calls must reach with the caller's arguments)."""

    def __init__(self, K, hidden=128, out=6, sh=False):
        super().__init__()
        nn = torch.nn
        self.config = StubConfig(0)
        self.config.appearance_model_sh = sh
        self.mlp = nn.Sequential(nn.Linear(K, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, out))
        self.calls = []

    def forward(self, gembedding, aembedding, color, viewdir=None):
        self.calls.append((gembedding, aembedding, color, viewdir))
        return "original"
