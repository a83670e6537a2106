"""Helpers of tests/test_dino_backbone.py, tests/golden/make_dino_golden.py and scripts/bench_dino_backbone.py: generated weights for a DINOv2
ViT-S/14 with 4 register tokens, a float64 restatement of its forward pass up to one block (the oracle), and a float32 torch module of the same
shape that stands in for the caller's backbone (wrapper tests, the benchmark's yardstick legs).

Weights come from one seed in the explicit order of `weight_names`, each drawn with numpy.random.default_rng: matrices N(0, 1 / fan_in), biases
and tokens 0.1 N, LayerNorm weights 1 + 0.1 N, LayerScale 0.5 + 0.25 N, the position embedding 0.1 N.  Nothing is stored: the fixture
tests/golden/dino_ref.npz holds recorded outputs of the reference's own class on these weights and inputs, and nothing else.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dino_ref.npz")
PATCH, EMBED, HEADS, HEAD_DIM, HIDDEN, DEPTH, REGS, POS_GRID = 14, 384, 6, 64, 1536, 12, 4, 37
LEAD = 1 + REGS
EPS = 1e-6
WEIGHT_SEED = 20240
CHANNEL_STRIDE = 8     # the fixture keeps every 8th channel of the float64 output, at all tokens

# patch grids h x w; N = 5 + h w straddles 64, 128 and 256
CASES = [
    dict(name="1x1", h=1, w=1, seed=1),
    dict(name="2x29", h=2, w=29, seed=2),
    dict(name="1x59", h=1, w=59, seed=3),
    dict(name="6x10", h=6, w=10, seed=4),
    dict(name="3x41", h=3, w=41, seed=5),
    dict(name="4x31", h=4, w=31, seed=6),
    dict(name="12x21", h=12, w=21, seed=7),
    dict(name="37x37", h=37, w=37, seed=8),
    dict(name="6x10-peaked", h=6, w=10, seed=9, peaked=True),
    dict(name="6x10-block2", h=6, w=10, seed=10, block=2),
    dict(name="5x7-offset", h=5, w=7, seed=11, offset=0.1, antialias=False),
]
for _c in CASES:
    _c.setdefault("peaked", False)
    _c.setdefault("block", HEADS - 1)
    _c.setdefault("offset", 0.0)
    _c.setdefault("antialias", True)


def case_id(c):
    return c["name"]


# ------------------------------------------------------------------------------------------------ weights and inputs
def weight_names(depth=DEPTH):
    names = ["patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed", "cls_token", "register_tokens", "mask_token"]
    for i in range(depth):
        b = f"blocks.{i}."
        names += [b + "norm1.weight", b + "norm1.bias", b + "attn.qkv.weight", b + "attn.qkv.bias", b + "attn.proj.weight", b + "attn.proj.bias",
                  b + "ls1.gamma", b + "norm2.weight", b + "norm2.bias", b + "mlp.fc1.weight", b + "mlp.fc1.bias", b + "mlp.fc2.weight",
                  b + "mlp.fc2.bias", b + "ls2.gamma"]
    return names + ["norm.weight", "norm.bias"]


def _shape_of(name):
    leaf = name.split(".", 2)[-1] if name.startswith("blocks.") else name
    return {"patch_embed.proj.weight": (EMBED, 3, PATCH, PATCH), "patch_embed.proj.bias": (EMBED,), "pos_embed": (1, 1 + POS_GRID * POS_GRID, EMBED),
            "cls_token": (1, 1, EMBED), "register_tokens": (1, REGS, EMBED), "mask_token": (1, EMBED),
            "attn.qkv.weight": (3 * EMBED, EMBED), "attn.qkv.bias": (3 * EMBED,), "attn.proj.weight": (EMBED, EMBED), "attn.proj.bias": (EMBED,),
            "mlp.fc1.weight": (HIDDEN, EMBED), "mlp.fc1.bias": (HIDDEN,), "mlp.fc2.weight": (EMBED, HIDDEN), "mlp.fc2.bias": (EMBED,)}.get(leaf, (EMBED,))


@functools.lru_cache(maxsize=None)
def _base_weights(seed=WEIGHT_SEED):
    rng = np.random.default_rng(seed)
    out = {}
    for name in weight_names():
        shape = _shape_of(name)
        z = rng.standard_normal(shape)
        if name.endswith(".gamma"):
            v = 0.5 + 0.25 * z
        elif ".norm" in name or name.startswith("norm."):
            v = 1.0 + 0.1 * z if name.endswith("weight") else 0.1 * z
        elif name.endswith(".weight"):
            v = z / math.sqrt(int(np.prod(shape[1:])))
        else:   # biases, tokens, the position embedding
            v = 0.1 * z
        out[name] = v.astype(np.float32)
    return out


def make_weights(peaked=False, seed=WEIGHT_SEED):
    """name -> float32 array (read-only: shared between cases).  peaked: block 0's qkv weight times 4, so that the scores of its attention span
    a wide range and the online softmax has to rescale."""
    w = dict(_base_weights(seed))
    if peaked:
        w["blocks.0.attn.qkv.weight"] = w["blocks.0.attn.qkv.weight"] * np.float32(4)
    return w


def state_dict(weights):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).clone() for k, v in weights.items()}


def make_image(c, B=1):
    """[B, 3, 14 h, 14 w] float32, N(0, 1): what a normalised frame looks like to the backbone."""
    rng = np.random.default_rng(1000 + c["seed"])
    return torch.from_numpy(rng.standard_normal((B, 3, PATCH * c["h"], PATCH * c["w"])).astype(np.float32))


# ------------------------------------------------------------------------------------------------ position embedding
def pos_embed_for(pos_embed, h, w, offset=0.0, antialias=True):
    """The position embedding of an h x w patch grid, [1 + h w, 384], in the dtype of `pos_embed` -- but interpolated in FLOAT32, as the model
    does whatever its own dtype is.  The parameter as it is for the grid it was made for."""
    pe = torch.as_tensor(pos_embed)
    n = pe.shape[1] - 1
    if h * w == n and h == w:
        return pe[0]
    m = int(math.sqrt(n))
    grid = pe[:, 1:].float().reshape(1, m, m, -1).permute(0, 3, 1, 2)
    how = {"scale_factor": (float(h + offset) / m, float(w + offset) / m)} if offset else {"size": (h, w)}
    grid = F.interpolate(grid, mode="bicubic", antialias=antialias, **how)
    assert tuple(grid.shape[-2:]) == (h, w)
    return torch.cat((pe[0, :1].float(), grid.permute(0, 2, 3, 1).reshape(h * w, -1)), 0).to(pe.dtype)


# ------------------------------------------------------------------------------------------------ the float64 oracle
def _ln64(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def attention64(qkv):
    """qkv [B, N, 3, 6, 64] (any float dtype) -> softmax(q k^T / 8) v as [B, N, 384], float64."""
    qkv = torch.as_tensor(qkv).double()
    B, N = qkv.shape[:2]
    q, k, v = qkv.reshape(B, N, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / 8.0
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhqk,bhkd->bqhd", p, v).reshape(B, N, EMBED)


def attention32_reference_formula(qkv):
    """The float32 statement sequence of the model's attention (q * scale @ k^T, softmax, @ v), on the CPU: its error is the tests' yardstick."""
    qkv = torch.as_tensor(qkv).float()
    B, N = qkv.shape[:2]
    q, k, v = qkv.reshape(B, N, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
    attn = ((q * HEAD_DIM ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, EMBED)


def oracle_features(weights, x, block=HEADS - 1, offset=0.0, antialias=True):
    """Float64 forward pass: the final norm applied to block `block`'s output, patch tokens only, as [B, 384, h, w] (a float64 tensor)."""
    W = {k: torch.as_tensor(v).double() for k, v in weights.items() if not k.startswith("blocks.") or int(k.split(".")[1]) <= block}
    x = torch.as_tensor(x).double()
    B, _, H, Wd = x.shape
    h, w = H // PATCH, Wd // PATCH
    patches = x.reshape(B, 3, h, PATCH, w, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, h * w, 3 * PATCH * PATCH)
    tok = patches @ W["patch_embed.proj.weight"].reshape(EMBED, -1).T + W["patch_embed.proj.bias"]
    pos = pos_embed_for(W["pos_embed"], h, w, offset, antialias)
    tok = tok + pos[1:]
    cls = (W["cls_token"].reshape(1, EMBED) + pos[:1]).expand(B, 1, EMBED)
    seq = torch.cat((cls, W["register_tokens"].expand(B, REGS, EMBED), tok), 1)
    for i in range(block + 1):
        g = lambda n: W[f"blocks.{i}.{n}"]
        y = _ln64(seq, g("norm1.weight"), g("norm1.bias"))
        o = attention64(y @ g("attn.qkv.weight").T + g("attn.qkv.bias"))
        seq = seq + g("ls1.gamma") * (o @ g("attn.proj.weight").T + g("attn.proj.bias"))
        y = _ln64(seq, g("norm2.weight"), g("norm2.bias"))
        z = y @ g("mlp.fc1.weight").T + g("mlp.fc1.bias")
        z = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
        seq = seq + g("ls2.gamma") * (z @ g("mlp.fc2.weight").T + g("mlp.fc2.bias"))
    out = _ln64(seq, W["norm.weight"], W["norm.bias"])[:, LEAD:]
    return out.reshape(B, h, w, EMBED).permute(0, 3, 1, 2).contiguous()


def run_oracle_case(c, B=1):
    return oracle_features(make_weights(c["peaked"]), make_image(c, B), c["block"], c["offset"], c["antialias"]).numpy()


# ------------------------------------------------------------------------------------------------ the fixture
def load_golden():
    """-> [(case, {"out64": [1, 48, h, w] float64, "ref32_dev": float, "max_abs": float})] in the order of CASES."""
    z = np.load(GOLDEN)
    return [(c, {"out64": z[c["name"] + "/out64"], "ref32_dev": float(z[c["name"] + "/ref32_dev"]), "max_abs": float(z[c["name"] + "/max_abs"])})
            for c in CASES]


# ------------------------------------------------------------------------------------------------ a float32 torch module of the same shape
class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.num_heads = HEADS
        self.qkv = nn.Linear(EMBED, 3 * EMBED)
        self.proj = nn.Linear(EMBED, EMBED)

    def forward(self, x, sdpa=False):
        B, N, Cn = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
        if sdpa:
            o = F.scaled_dot_product_attention(q, k, v)
        else:   # materialised: what runs where no fused attention is importable
            o = ((q * HEAD_DIM ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1) @ v
        return self.proj(o.transpose(1, 2).reshape(B, N, Cn))


class _Mlp(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(EMBED, HIDDEN), nn.GELU(), nn.Linear(HIDDEN, EMBED)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _LayerScale(nn.Module):
    def __init__(self):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(EMBED))

    def forward(self, x):
        return x * self.gamma


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(EMBED, eps=EPS), _Attention(), _LayerScale()
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(EMBED, eps=EPS), _Mlp(), _LayerScale()

    def forward(self, x, sdpa=False):
        x = x + self.ls1(self.attn(self.norm1(x), sdpa))
        return x + self.ls2(self.mlp(self.norm2(x)))


class _PatchEmbed(nn.Module):
    """`proj` is the caller's 14 x 14 stride-14 convolution.  `conv=False` evaluates it as patches times the weight matrix (one F.linear): the
    same sums, without the convolution library -- what the tests use, so that they leave no state of that library behind in the process."""

    def __init__(self, conv):
        super().__init__()
        self.proj = nn.Conv2d(3, EMBED, kernel_size=PATCH, stride=PATCH)
        self.norm = nn.Identity()
        self.conv = conv

    def forward(self, x):
        if self.conv:
            return self.proj(x).flatten(2).transpose(1, 2)
        B, Cn, H, Wd = x.shape
        h, w = H // PATCH, Wd // PATCH
        patches = x[:, :, :h * PATCH, :w * PATCH].reshape(B, Cn, h, PATCH, w, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B, h * w, Cn * PATCH * PATCH)
        return F.linear(patches, self.proj.weight.reshape(EMBED, -1), self.proj.bias)


class TorchBackbone(nn.Module):
    """A ViT-S/14 with 4 register tokens in plain float32 torch, with the attribute names a caller's DinoVisionTransformer has (so that its
    state dict takes `state_dict(make_weights())`).  `stop_early`: leave the block loop after the last block that is asked for; `sdpa`:
    F.scaled_dot_product_attention instead of the materialised softmax.  Both off: what the caller runs today, all 12 blocks.  `conv`: the
    patch embedding through F.conv2d, as the caller runs it (the benchmark), instead of one F.linear over the patches (the tests)."""

    def __init__(self, weights=None, offset=0.0, antialias=True, stop_early=False, sdpa=False, conv=False):
        super().__init__()
        self.patch_size, self.num_heads, self.embed_dim, self.num_register_tokens = PATCH, HEADS, EMBED, REGS
        self.interpolate_offset, self.interpolate_antialias, self.chunked_blocks = offset, antialias, False
        self.stop_early, self.sdpa = stop_early, sdpa
        self.patch_embed = _PatchEmbed(conv)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, EMBED))
        self.register_tokens = nn.Parameter(torch.zeros(1, REGS, EMBED))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + POS_GRID * POS_GRID, EMBED))
        self.mask_token = nn.Parameter(torch.zeros(1, EMBED))
        self.blocks = nn.ModuleList([_Block() for _ in range(DEPTH)])
        self.norm = nn.LayerNorm(EMBED, eps=EPS)
        self.calls = 0
        if weights is not None:
            self.load_state_dict(state_dict(weights))
        for p in self.parameters():
            p.requires_grad = False

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        assert not return_class_token and norm and reshape
        self.calls += 1
        take = list(range(DEPTH - n, DEPTH)) if isinstance(n, int) else list(n)
        B, _, H, Wd = x.shape
        h, w = H // PATCH, Wd // PATCH
        pos = pos_embed_for(self.pos_embed, h, w, self.interpolate_offset, self.interpolate_antialias)
        tok = self.patch_embed(x) + pos[1:]
        cls = (self.cls_token[0] + pos[:1]).expand(B, 1, EMBED)
        seq = torch.cat((cls, self.register_tokens.expand(B, REGS, EMBED), tok), 1)
        outs = []
        for i, blk in enumerate(self.blocks):
            seq = blk(seq, self.sdpa)
            if i in take:
                outs.append(self.norm(seq)[:, LEAD:].reshape(B, h, w, EMBED).permute(0, 3, 1, 2).contiguous())
            if self.stop_early and i >= max(take):
                break
        return tuple(outs)


# ------------------------------------------------------------------------------------------------ a stand-in UncertaintyModel
def stand_in_uncertainty_model(backbone, training=True):
    """-> (model, its class): a subclass of tests/uncertainty_lib.StandInModel (whose `_get_dino_cached` is the caller's, statement for statement)
    around `backbone`.  A class of its own, so that what a test swaps on it stays off the shared one."""
    import uncertainty_lib as U

    class Model(U.StandInModel):
        def _compute_losses(self, gt, prediction, prefix='', _cache_entry=None):
            raise AssertionError("a covered call reached the original method")

    model = Model({"C": EMBED, "seed": 77, "training": training, "init": "clamp"})
    model.backbone = backbone
    model.patch_size = backbone.patch_size
    return model, Model
