"""Helpers of tests/test_lpips.py, tests/golden/make_lpips_golden.py and scripts/bench_lpips.py: generated weights for LPIPS v0.1 on the AlexNet
and VGG16 trunks, a float64 restatement of its forward pass with the five taps (the oracle), and a float32 torch module of the reference's
shape that stands in for the caller's `LPIPS` object (wrapper tests, the benchmark's yardstick legs).

Weights come from one seed per net in the explicit order of `weight_names`, each drawn with numpy.random.default_rng: convolutions
N(0, 2 / fan_in), biases 0.1 N, `lin` weights |N| LIN_K / C (non-negative, as the trained ones are; LIN_K puts the cases' values between 0.1
and 1).  The scaling layer's buffers are the reference's constants.  Nothing is stored: the fixture tests/golden/lpips_ref.npz holds recorded
outputs of the reference's own class on these weights and inputs, and nothing else.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lpips_ref.npz")
WEIGHT_SEED = {"alex": 31001, "vgg": 31002}
LIN_K = 64.0
CHANNEL_STRIDE = 16    # the fixture keeps every 16th channel of the float64 taps of the first argument's images
TAPS = 5
EPS = 1e-10
MIN_SIDE = {"alex": 31, "vgg": 16}
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# The trunks as torchvision's `.features` lists them: ("conv", cin, cout, window, stride, pad) / ("relu",) / ("pool", window), and the index in
# that list where each of the reference's five slices ends (exclusive).
_c3 = lambda cin, cout: ("conv", cin, cout, 3, 1, 1)
FEATURES = {
    "alex": [("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3), _c3(192, 384), ("relu",),
             _c3(384, 256), ("relu",), _c3(256, 256), ("relu",), ("pool", 3)],
    "vgg": [_c3(3, 64), ("relu",), _c3(64, 64), ("relu",), ("pool", 2), _c3(64, 128), ("relu",), _c3(128, 128), ("relu",), ("pool", 2),
            _c3(128, 256), ("relu",), _c3(256, 256), ("relu",), _c3(256, 256), ("relu",), ("pool", 2),
            _c3(256, 512), ("relu",), _c3(512, 512), ("relu",), _c3(512, 512), ("relu",), ("pool", 2),
            _c3(512, 512), ("relu",), _c3(512, 512), ("relu",), _c3(512, 512), ("relu",), ("pool", 2)],
}
SLICE_ENDS = {"alex": [2, 5, 8, 10, 12], "vgg": [4, 9, 16, 23, 30]}
CHANNELS = {"alex": [64, 192, 384, 256, 256], "vgg": [64, 128, 256, 512, 512]}

CASES = [
    dict(net="alex", H=31, W=31, seed=1),       # the minimum: taps 1 to 4 are 1 x 1
    dict(net="alex", H=32, W=35, seed=2),       # the first convolution's stride leaves rows and columns unread
    dict(net="alex", H=35, W=67, seed=3),
    dict(net="alex", H=64, W=48, seed=4),
    dict(net="alex", H=97, W=130, seed=5),
    dict(net="alex", H=131, W=259, seed=6),
    dict(net="vgg", H=16, W=16, seed=7),        # the minimum
    dict(net="vgg", H=17, W=33, seed=8),        # odd sizes through every pool
    dict(net="vgg", H=31, W=47, seed=9),
    dict(net="vgg", H=50, W=70, seed=10),
    dict(net="vgg", H=64, W=96, seed=11),
    dict(net="alex", H=31, W=31, seed=12, B=2),   # batches: a 128-pixel tile of the implicit GEMM then spans images
    dict(net="alex", H=31, W=31, seed=13, B=3),
    dict(net="vgg", H=17, W=33, seed=14, B=2),
    dict(net="vgg", H=17, W=33, seed=15, B=3),
]
for _c in CASES:
    _c.setdefault("B", 1)
    _c["name"] = f"{_c['net']}-{_c['H']}x{_c['W']}" + (f"-B{_c['B']}" if _c["B"] > 1 else "")


def case_id(c):
    return c["name"]


# ------------------------------------------------------------------------------------------------ weights and inputs
def conv_positions(net):
    return [i for i, f in enumerate(FEATURES[net]) if f[0] == "conv"]


def _slice_of(net, index):
    return next(s for s, end in enumerate(SLICE_ENDS[net]) if index < end)


def weight_names(net):
    """The reference LPIPS object's state dict, in its own order of registration."""
    names = ["scaling_layer.shift", "scaling_layer.scale"]
    for i in conv_positions(net):
        names += [f"net.slice{_slice_of(net, i) + 1}.{i}.weight", f"net.slice{_slice_of(net, i) + 1}.{i}.bias"]
    names += [f"lin{l}.model.1.weight" for l in range(TAPS)]
    return names + [f"lins.{l}.model.1.weight" for l in range(TAPS)]


@functools.lru_cache(maxsize=None)
def make_weights(net):
    """-> {name: float32 tensor}; `lins.l` names hold the same tensors as `linl` (the reference registers each layer twice)."""
    rng = np.random.default_rng(WEIGHT_SEED[net])
    out = {"scaling_layer.shift": torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1),
           "scaling_layer.scale": torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1)}
    for i in conv_positions(net):
        _, cin, cout, k, _, _ = FEATURES[net][i]
        base = f"net.slice{_slice_of(net, i) + 1}.{i}."
        out[base + "weight"] = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
        out[base + "bias"] = torch.from_numpy((0.1 * rng.standard_normal(cout)).astype(np.float32))
    for l, cn in enumerate(CHANNELS[net]):
        w = torch.from_numpy((np.abs(rng.standard_normal((1, cn, 1, 1))) * LIN_K / cn).astype(np.float32))
        out[f"lin{l}.model.1.weight"] = w
    for l in range(TAPS):
        out[f"lins.{l}.model.1.weight"] = out[f"lin{l}.model.1.weight"]
    assert list(out) == weight_names(net)
    return out


def make_images(c):
    """-> (pred, gt): float32 [B, 3, H, W], independent, uniform on [-0.05, 1.05]: a twentieth of the values are clipped at either end."""
    rng = np.random.default_rng(5000 + c["seed"])
    draw = lambda: torch.from_numpy(rng.uniform(-0.05, 1.05, (c["B"], 3, c["H"], c["W"])).astype(np.float32))
    return draw(), draw()


# ------------------------------------------------------------------------------------------------ the float64 oracle
def oracle_taps(weights, net, x):
    """x [N, 3, H, W] float32 in the caller's [0, 1] convention -> the five taps in float64.  The caller's chain: clip, * 2, - 1, the scaling
    layer, then the trunk up to the ReLU that ends each slice."""
    w = {k: v.double() for k, v in weights.items()}
    h = x.double().clamp(0.0, 1.0) * 2.0 - 1.0
    h = (h - w["scaling_layer.shift"]) / w["scaling_layer.scale"]
    taps = []
    for i, f in enumerate(FEATURES[net][:SLICE_ENDS[net][-1]]):
        if f[0] == "conv":
            base = f"net.slice{_slice_of(net, i) + 1}.{i}."
            h = F.conv2d(h, w[base + "weight"], w[base + "bias"], stride=f[4], padding=f[5])
        elif f[0] == "relu":
            h = F.relu(h)
        else:
            h = F.max_pool2d(h, f[1], 2)
        if i + 1 in SLICE_ENDS[net]:
            taps.append(h)
    return taps


def oracle_head(f0, f1, lin):
    """One tap: float64 features [B, C, h, w] of both images, lin [1, C, 1, 1] -> [B]."""
    g0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    g1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    return ((g0 - g1).pow(2) * lin.double()).sum(1).mean((1, 2))


def oracle(weights, net, pred, gt):
    """-> (total [B], layers [B, 5], taps of pred, taps of gt), all float64."""
    t0, t1 = oracle_taps(weights, net, pred), oracle_taps(weights, net, gt)
    layers = torch.stack([oracle_head(a, b, weights[f"lin{l}.model.1.weight"]) for l, (a, b) in enumerate(zip(t0, t1))], dim=1)
    return layers.sum(1), layers, t0, t1


@functools.lru_cache(maxsize=None)
def run_oracle_case(name):
    c = next(c for c in CASES if c["name"] == name)
    pred, gt = make_images(c)
    total, layers, t0, t1 = oracle(make_weights(c["net"]), c["net"], pred, gt)
    return total.numpy(), layers.numpy(), [t.numpy() for t in t0], [t.numpy() for t in t1]


def load_golden():
    """-> [(case, {key: array})] in the order of CASES."""
    data = np.load(GOLDEN)
    out = []
    for c in CASES:
        prefix = c["name"] + "/"
        out.append((c, {k[len(prefix):]: data[k] for k in data.files if k.startswith(prefix)}))
    return out


# ------------------------------------------------------------------------------------------------ a stand-in of the caller's module
class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1))

    def forward(self, x):
        return (x - self.shift) / self.scale


class _Lin(nn.Module):
    def __init__(self, cn):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(cn, 1, 1, bias=False))

    def forward(self, x):
        return self.model(x)


def feature_layers(net):
    """The trunk as torchvision builds its `.features`: an nn.Sequential with in-place ReLUs."""
    mods = []
    for f in FEATURES[net]:
        if f[0] == "conv":
            mods.append(nn.Conv2d(f[1], f[2], f[3], stride=f[4], padding=f[5]))
        elif f[0] == "relu":
            mods.append(nn.ReLU(inplace=True))
        else:
            mods.append(nn.MaxPool2d(f[1], 2))
    return nn.Sequential(*mods)


class _Trunk(nn.Module):
    def __init__(self, net):
        super().__init__()
        feats, start = feature_layers(net), 0
        for s, end in enumerate(SLICE_ENDS[net]):
            sl = nn.Sequential()
            for i in range(start, end):
                sl.add_module(str(i), feats[i])
            setattr(self, f"slice{s + 1}", sl)
            start = end
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, x):
        outs = []
        for s in range(TAPS):
            x = getattr(self, f"slice{s + 1}")(x)
            outs.append(x)
        return outs


class StandInLPIPS(nn.Module):
    """A float32 module with the attributes, state dict names and forward signature of the reference's `LPIPS(net=..., version="0.1")`."""

    def __init__(self, net="alex", weights=None, version="0.1", lpips=True, spatial=False):
        super().__init__()
        self.pnet_type, self.version, self.lpips, self.spatial = net, version, lpips, spatial
        key = "vgg" if net in ("vgg", "vgg16") else net
        self.chns = CHANNELS[key]
        self.L = TAPS
        self.scaling_layer = _Scaling()
        self.net = _Trunk(key)
        for l, cn in enumerate(self.chns):
            setattr(self, f"lin{l}", _Lin(cn))
        self.lins = nn.ModuleList([getattr(self, f"lin{l}") for l in range(TAPS)])
        if weights is not None:
            self.load_state_dict(weights, strict=True)
        self.eval()
        self.calls = 0

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        self.calls += 1
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        f0, f1 = self.net(self.scaling_layer(in0)), self.net(self.scaling_layer(in1))
        res = []
        for l in range(TAPS):
            g0 = f0[l] / (torch.sqrt(torch.sum(f0[l] ** 2, dim=1, keepdim=True)) + EPS)
            g1 = f1[l] / (torch.sqrt(torch.sum(f1[l] ** 2, dim=1, keepdim=True)) + EPS)
            res.append(self.lins[l]((g0 - g1) ** 2).mean([2, 3], keepdim=True))
        val = sum(res[1:], res[0])
        return (val, res) if retPerLayer else val


def stand_in_evaluation_module(nets=(), device=None):
    """A module object with the names `wg_integration.fuse_evaluation_lpips` touches: `_LPIPS_CACHE`, `_lpips` (the statements of the caller's
    function, except that a missing network is built from the generated weights instead of downloaded), `lpips`, `lpips_vgg`, `compute_metrics`.  `device` (default: the HIP device where there is one) is where the caller's own forward pass runs."""
    import types
    m = types.ModuleType("stand_in_evaluation")
    m._LPIPS_CACHE = {net: StandInLPIPS(net, make_weights(net)) for net in nets}
    m.built, m.original_calls, m.device = [], [], device

    def _lpips(a, b, net, version="0.1"):
        m.original_calls.append((a, b, net, version))
        assert a.shape == b.shape and a.dtype.kind == "f" and b.dtype.kind == "f"
        lp_net = m._LPIPS_CACHE.get(net)
        if lp_net is None:
            lp_net = m._LPIPS_CACHE[net] = StandInLPIPS(net, make_weights(net), version=version)
            m.built.append(net)
        device = torch.device(m.device if m.device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        batch_shape, img_shape = a.shape[:-3], a.shape[-3:]
        prepare = lambda v: torch.from_numpy(np.clip(v, 0, 1).astype(np.float32)).float().view(-1, *img_shape).permute(0, 3, 1, 2).mul_(2).sub_(1).to(device)
        with torch.no_grad():
            out = lp_net.to(device).forward(prepare(a), prepare(b))
        return out.detach().cpu().numpy().reshape(batch_shape)

    m._lpips = _lpips
    m.lpips = lambda a, b: m._lpips(a, b, net="alex")
    m.lpips_vgg = lambda a, b: m._lpips(a, b, net="vgg")

    def compute_metrics(pred, gt, *, reduce=True, run_lpips_vgg=False):
        red = (lambda x: x.mean().item()) if reduce else (lambda x: x)
        pred = pred[..., :gt.shape[-1]].astype(np.float32)
        gt = gt.astype(np.float32)
        out = {"mse": red(((pred - gt) ** 2).mean((-1, -2, -3))), "lpips": red(m.lpips(gt, pred))}
        if run_lpips_vgg:
            out["lpips_vgg"] = red(m.lpips_vgg(gt, pred))
        return out

    m.compute_metrics = compute_metrics
    return m
