"""Shared by tests/test_densify_prune.py and tests/golden/make_densify_golden.py: the inputs of a densification step by seed, and a float64
restatement of GaussianModel.densify_and_prune / reset_opacity (wildgaussians/method.py:1249-1468) with rounding bounds that follow from the
arithmetic (u = 2^-24).  numpy only.

Decisions.  g = xyz_grad / denom and ga = xyz_gradient_accum_abs / denom are single correctly rounded float32 divisions on every side, so they
are formed here in float32 and are exact.  The other decision inputs -- exp(scale), sigmoid(opacity) -- differ between implementations in
their last bits; `make_inputs` keeps every one of them a relative GAP = 3e-4 away from its threshold by construction, and `restate` asserts a
gap of 1e-4 (three orders above a float32 exp / sigmoid disagreement), so that decisions can be compared exactly, nothing left out.

Bounds (derivations; "rel" is a relative error, transcendental functions are taken as 2-ulp functions = 4 u rel):
  Q = lerp(a, b, w), a, b adjacent order statistics, w exact: the difference, the product (or (1 - w) and a product) and the sum round:
      |err| <= u (|Q| + 3 |b - a|); exact when a == b.
  child xyz = R(q) . (z * exp(s)) + xyz:  exp 4 u, product u -> samples 5 u rel.  Quaternion: |r|^2 4 u, sqrt 3 u, reciprocal 4 u, component 5 u,
      the second normalisation (norm 3 u + division u) 9 u.  R entry: products of two components 19 u, sum of two (|xy| + |rz| <= 1) 20 u, doubled
      and taken from 1: <= 41 u absolute; take 42 u.  Term R_ik samp_k: (42 + 5 + 1) u |samp_k|; the two additions of the 3-term sum u each of at
      most sum |samp_k|; the last addition u |xyz_new|:
      |err_i| <= 50 u sum_k |z_k| exp(s_k) + 2 u |xyz_new_i|.
  child scale = log(exp(s) / float32(1.6)):  exp 4 u, division u -> argument 5 u rel = 5 u absolute after the log, log 4 u rel:
      |err| <= 6 u + 4 u |scale_new|.
  reset opacity y = logit(min(sigmoid(o) c1, 0.01) / c2): sigmoid 6 u (exp, sum, reciprocal); t = exp(s) 4 u, t^2 9 u, t^2 + f^2 10 u,
      products of three 29 u / 32 u, quotient 62 u, sqrt -> c1 32 u; sigmoid c1 39 u (the min keeps it); filtered scale sqrt(t^2 + f^2) 6 u, squared
      13 u, + f^2 14 u, products 41 u / 44 u, quotient 86 u, sqrt -> c2 44 u; x = ./c2 84 u; 1 - x: (84 u x + u) / (1 - x) rel; the quotient u; log 4 u rel:
      |err| <= 85 u + (84 u x + u) / (1 - x) + 4 u |y|.
"""
import numpy as np

U = 2.0 ** -24
GAP_BUILD, GAP = 3e-4, 1e-4
F32 = np.float32
DEFAULTS = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, percent_dense=0.01, enable_size_pruning=True, use_abs_gradient=True)
PARAMS = ("xyz", "features_dc", "features_rest", "scales", "rotations", "opacities", "embeddings")
BUFFERS = ("xyz_grad", "denom", "filter_3D", "max_radii2D", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max")


def thresholds(p):
    """The thresholds as the reference's float32 comparisons see them: Python forms the products in double, torch rounds them to float32."""
    return dict(max_grad=float(F32(p["max_grad"])), min_opacity=float(F32(p["min_opacity"])),
                dense=float(F32(p["percent_dense"] * p["extent"])), size=float(F32(0.1 * p["extent"])))


def _near(v, t):
    return np.abs(v / t - 1.0) < GAP_BUILD


def make_inputs(P, seed, sh_degree=1, n_embed=6, ga_mode="grid", params=None):
    """-> dict of float32 arrays (PARAMS, BUFFERS, "<param>.exp_avg", "<param>.exp_avg_sq").  About 10 % hot by g, scales spread over both
    sides of percent_dense * extent with a tail beyond 0.1 * extent (and beyond 1.6 x that: children that are pruned for size), 5 % faint,
    3 % never seen (denom = 0: NaN statistics).  ga_mode "grid": ga takes a few dozen exactly representable values (ties at Q);
    "continuous": all distinct (Q strictly between two order statistics).  features_dc[:, 0] is the row index."""
    p = dict(DEFAULTS, **(params or {}))
    t = thresholds(p)
    rng = np.random.default_rng(seed)
    d = {}
    d["xyz"] = (rng.standard_normal((P, 3)) * p["extent"] * 0.3).astype(F32)
    d["features_dc"] = rng.standard_normal((P, 3)).astype(F32)
    d["features_dc"][:, 0] = np.arange(P, dtype=F32)
    nrest = 3 * ((sh_degree + 1) ** 2 - 1)
    if nrest:
        d["features_rest"] = rng.standard_normal((P, nrest)).astype(F32)
    if n_embed:
        d["embeddings"] = rng.standard_normal((P, n_embed)).astype(F32)
    d["rotations"] = rng.standard_normal((P, 4)).astype(F32)
    # scales: median at the clone / split threshold, sigma 1.3 in log space: ~4 % beyond 0.1 extent, ~1.5 % beyond 1.6 x that
    s = (np.log(t["dense"]) + 1.3 * rng.standard_normal((P, 1)) + 0.3 * rng.standard_normal((P, 3))).astype(F32)
    for _ in range(8):
        m = np.exp(s.astype(np.float64)).max(axis=1)
        bad = _near(m, t["dense"]) | _near(m, t["size"]) | _near(m / float(F32(1.6)), t["size"])
        if not bad.any():
            break
        s[bad] = (s[bad].astype(np.float64) + 0.002).astype(F32)
    d["scales"] = s
    o = rng.uniform(0.02, 0.95, (P, 1))
    faint = rng.uniform(size=(P, 1)) < 0.05
    o = np.where(faint, rng.uniform(0.0005, 0.0049, (P, 1)), o)
    o = np.log(o / (1 - o)).astype(F32)
    for _ in range(8):
        bad = _near(1.0 / (1.0 + np.exp(-o.astype(np.float64))), t["min_opacity"])
        if not bad.any():
            break
        o[bad] = (o[bad].astype(np.float64) + 0.002).astype(F32)
    d["opacities"] = o
    denom = rng.integers(1, 9, (P, 1)).astype(F32)
    denom[rng.uniform(size=(P, 1)) < 0.03] = 0.0
    g = p["max_grad"] * np.exp(1.0 * rng.standard_normal((P, 1)) - 1.28)   # ~10 % at or above max_grad
    xg = (g * denom).astype(F32)
    for _ in range(8):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = (xg / denom).astype(np.float64)
        bad = np.isfinite(q) & _near(np.where(np.isfinite(q) & (q > 0), q, 1.0), t["max_grad"])
        if not bad.any():
            break
        xg[bad] = (xg[bad].astype(np.float64) * 1.001).astype(F32)
    d["xyz_grad"], d["denom"] = xg, denom
    if ga_mode == "grid":   # k 2^-16 times an integer <= 8: the product and the quotient are exact in float32
        k = np.minimum(rng.geometric(0.12, (P, 1)), 60).astype(np.float64)
        d["xyz_gradient_accum_abs"] = (k * 2.0 ** -16 * denom).astype(F32)
    else:
        d["xyz_gradient_accum_abs"] = (p["max_grad"] * 2.0 * np.exp(rng.standard_normal((P, 1))) * denom).astype(F32)
    d["xyz_gradient_accum_abs_max"] = rng.uniform(0.0, 1e-3, (P, 1)).astype(F32)
    d["filter_3D"] = rng.uniform(0.001, 0.01, (P, 1)).astype(F32)
    d["max_radii2D"] = rng.integers(0, 40, (P,)).astype(F32)
    for k in PARAMS:
        if k in d:
            d[k + ".exp_avg"] = (rng.standard_normal(d[k].shape) * 1e-3).astype(F32)
            d[k + ".exp_avg_sq"] = (rng.uniform(1e-8, 1e-5, d[k].shape)).astype(F32)
    return d


def quantile64(values32, q=None, hot=None):
    """The selection of wg_quantile / torch.quantile on float32 values: -> dict(Q, bound, lo, hi, a, b, w, ratio).  q: a float (rounded to float32
    for n <= 2^24, as torch does), or None with `hot` the integer count from which ratio and q = 1 - ratio are formed."""
    v = np.asarray(values32, F32).reshape(-1)
    n = v.shape[0]
    ratio = None
    if n <= 2 ** 24:
        if q is None:
            ratio = F32(hot) / F32(n)
            q32 = F32(1.0) - ratio
        else:
            q32 = F32(q)
        rank = F32(q32 * F32(n - 1))
        lo, hi = int(np.floor(rank)), int(np.ceil(rank))
        w = float(rank - F32(lo))
    else:
        if q is None:
            ratio = hot / n
            q = 1.0 - ratio
        rank = q * (n - 1)
        lo, hi = int(np.floor(rank)), int(np.ceil(rank))
        w = rank - lo
    lo, hi = min(lo, n - 1), min(hi, n - 1)
    v = np.partition(v, sorted({lo, hi}))   # the two order statistics, without a full sort
    a, b = float(v[lo]), float(v[hi])
    Q = a + w * (b - a)
    return dict(Q=Q, bound=0.0 if a == b else U * (abs(Q) + 3 * abs(b - a)) * (1 + 2.0 ** -20), lo=lo, hi=hi, a=a, b=b, w=w,
                ratio=None if ratio is None else float(ratio), n=n)


def rotation64(r):
    q = r.astype(np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)   # noqa: E702
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)   # noqa: E702
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)   # noqa: E702
    return R


def restate(d, params=None, noise=None):
    """The reference's statements in float64 on the float32 inputs.  -> dict: ratio, n_hot, Q, Q_bound, clone / split masks, origin [P_new, 2],
    counts (n_cloned, n_split, n_pruned), n_out, and with `noise` ([2 S, 3]) child_xyz / child_xyz_bound / child_scales / child_scales_bound
    for ALL 2 S children, copy-major, with child_kept.  Asserts that no decision lies within GAP of its threshold."""
    p = dict(DEFAULTS, **(params or {}))
    t = thresholds(p)
    P = d["xyz"].shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (d["xyz_grad"] / d["denom"]).reshape(-1)
        g = np.where(np.isnan(g), F32(0), g).astype(np.float64)
    hot_g = np.abs(g) >= t["max_grad"]
    out = dict(n_hot=int(hot_g.sum()), nan_stats=int((d["denom"] == 0).sum()))
    fin = np.isfinite(g) & (g > 0)
    assert not (np.abs(g[fin] / t["max_grad"] - 1.0) < GAP).any(), "a gradient within the gap of max_grad"
    hot_clone, hot_split = hot_g.copy(), g >= t["max_grad"]
    if p["use_abs_gradient"]:
        with np.errstate(invalid="ignore", divide="ignore"):
            ga = (d["xyz_gradient_accum_abs"] / d["denom"]).reshape(-1)
            ga = np.where(np.isnan(ga), F32(0), ga)
        qs = quantile64(ga, hot=out["n_hot"])
        ga = ga.astype(np.float64)
        if qs["bound"] > 0:   # Q lies between two adjacent order statistics: nothing may sit within its rounding error
            assert not (np.abs(ga - qs["Q"]) <= 2 * qs["bound"]).any(), "a value within Q's rounding error of Q"
        out.update(Q=qs["Q"], Q_bound=qs["bound"], ratio=qs["ratio"], q_stats=qs, ties_at_Q=int((ga == qs["Q"]).sum()))
        hot_clone |= np.abs(ga) >= qs["Q"]
        hot_split |= ga >= qs["Q"]
    else:
        out.update(Q=None, Q_bound=0.0, ratio=float(F32(out["n_hot"]) / F32(P)) if P else 0.0)
    rs = np.exp(d["scales"].astype(np.float64))
    m = rs.max(axis=1)
    sig = (1.0 / (1.0 + np.exp(-d["opacities"].astype(np.float64)))).reshape(-1)
    mc = m / float(F32(1.6))
    for v, thr, what in ((m, t["dense"], "scale vs percent_dense * extent"), (sig, t["min_opacity"], "opacity vs min_opacity")) + \
            (((m, t["size"], "scale vs 0.1 * extent"), (mc, t["size"], "child scale vs 0.1 * extent")) if p["enable_size_pruning"] else ()):
        assert not (np.abs(v / thr - 1.0) < GAP).any(), "a decision within the gap: " + what
    clone, split = hot_clone & (m <= t["dense"]), hot_split & (m > t["dense"])
    assert not (clone & split).any()
    faint = sig < t["min_opacity"]
    prune_self = faint | (p["enable_size_pruning"] & (m > t["size"]))
    prune_child = faint | (p["enable_size_pruning"] & (mc > t["size"]))
    idx = np.arange(P)
    segs = [idx[~split & ~prune_self], idx[clone & ~prune_self], idx[split & ~prune_child], idx[split & ~prune_child]]
    out["origin"] = np.concatenate([np.stack([s, np.full_like(s, k)], axis=1) for k, s in enumerate(segs)]).astype(np.int32)
    out["n_out"] = tuple(len(s) for s in segs)
    S = int(split.sum())
    out["counts"] = (int(clone.sum()), S, P + int(clone.sum()) + S - sum(out["n_out"]))
    out.update(clone=clone, split=split, prune_self=prune_self, prune_child=prune_child,
               pruned_originals=int((prune_self & ~split).sum()), pruned_children=2 * int((split & prune_child).sum()))
    if noise is not None:
        assert noise.shape == (2 * S, 3)
        par = np.concatenate([idx[split], idx[split]])
        samp = noise.astype(np.float64) * rs[par]
        R = rotation64(d["rotations"][par])
        xyz = np.einsum("nij,nj->ni", R, samp) + d["xyz"][par].astype(np.float64)
        out["child_parent"], out["child_kept"] = par, ~prune_child[par]
        out["child_xyz"] = xyz
        out["child_xyz_bound"] = 50 * U * np.abs(samp).sum(axis=1, keepdims=True) + 2 * U * np.abs(xyz)
        sc = np.log(rs[par] / float(F32(1.6)))
        out["child_scales"], out["child_scales_bound"] = sc, 6 * U + 4 * U * np.abs(sc)
    return out


def reset_opacity64(opac, scales, filt):
    """-> (y, bound): reset_opacity's new raw opacities (method.py:1252-1266) in float64, with the bound of the module docstring."""
    o, s, f = opac.astype(np.float64).reshape(-1), scales.astype(np.float64), filt.astype(np.float64).reshape(-1, 1)
    t2 = np.exp(s) ** 2
    c1 = np.sqrt(t2.prod(axis=1) / (t2 + f ** 2).prod(axis=1))
    cur = np.minimum(1.0 / (1.0 + np.exp(-o)) * c1, float(F32(0.01)))
    sc2 = t2 + f ** 2            # the square of the filtered scales the reference starts from
    c2 = np.sqrt(sc2.prod(axis=1) / (sc2 + f ** 2).prod(axis=1))
    x = cur / c2
    y = np.log(x / (1.0 - x))
    return y, 85 * U + (84 * U * x + U) / (1.0 - x) + 4 * U * np.abs(y)
