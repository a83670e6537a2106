"""Fused frozen DINOv2 ViT-S/14 feature extractor (include/wg_dino.h, wg_fused_dino, apply_optins(uncertainty_backbone=True)) against the
reference's DinoVisionTransformer.get_intermediate_layers(x, n=[k], reshape=True) (wildgaussians/dinov2.py:789-813).

Oracle: tests/dino_lib.py's float64 restatement, pinned (on the CPU) to the float64 outputs recorded from the reference's own class in
tests/golden/dino_ref.npz (every 8th channel, all tokens).  Weights and images are regenerated from seeds.
Tolerance, per case: max |fused - float64| over the WHOLE tensor <= 4 * max(ref32_dev, floor); ref32_dev = the reference's own recorded
max |float32 - float64| on that input, floor = 16 float32 ulps of the output's largest magnitude (the form and the factor of
tests/test_uncertainty.py).  The attention stage alone is held the same way, ref32_dev being the error of the reference's float32 statement
sequence (q * scale @ k^T, softmax, @ v) on the same input, computed here on the CPU.
Shapes (tests/dino_lib.CASES): token counts N = 5 + h w of 6, 63, 64, 65, 128, 129, 257 and 1374 (37 x 37: the position embedding as it is);
one case whose block-0 scores are 16 times wider (the online softmax has to rescale), one at block 2, one with the other position-embedding
branch (scale_factor, no antialiasing).  The products have two tilings chosen by size; 1374 tokens take both, and both are forced at 6, 129
and 1374 tokens and held to the bits of the automatic choice.
Measured on an MI355X (profiles/dino_backbone/accuracy.json): ratios of max(ref32_dev, floor) between 0.46 and 0.90 over the eleven cases."""
import ctypes as C
import functools
import gc
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dino_lib as L  # noqa: E402
import wg_fused_dino as D  # noqa: E402

GOLDEN = L.load_golden()
IDS = [L.case_id(c) for c, _ in GOLDEN]
INDEX = list(range(len(GOLDEN)))
ULP16 = lambda largest: 16 * float(np.spacing(np.float32(largest)))
OTHERS_OFF = dict(ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False)
BAD = -1   # WG_ERR_INVALID_ARGUMENT


def gate(ref32_dev, largest):
    return 4 * max(ref32_dev, ULP16(largest))


# ---------------------------------------------------------------- CPU: the fixture, the oracle, the C-ABI, the opt-in's logic

def test_fixture_holds_the_cases_of_the_helper_and_stays_small():
    wanted = {6, 63, 64, 65, 128, 129, 257, 1374}
    assert wanted <= {L.LEAD + c["h"] * c["w"] for c, _ in GOLDEN}
    assert sum(c["peaked"] for c, _ in GOLDEN) == 1 and sum(c["block"] == 2 for c, _ in GOLDEN) == 1
    assert sum(c["offset"] == 0.1 and not c["antialias"] for c, _ in GOLDEN) == 1
    for c, a in GOLDEN:
        assert a["out64"].dtype == np.float64 and a["out64"].shape == (1, L.EMBED // L.CHANNEL_STRIDE, c["h"], c["w"])
        assert 0 < a["ref32_dev"] < 1e-4 and 1 < a["max_abs"] < 10
    assert os.path.getsize(L.GOLDEN) < 1_000_000
    assert L.weight_names()[:3] == ["patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed"] and len(L.weight_names()) == 6 + 14 * 12 + 2


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_float64_oracle_reproduces_the_recorded_reference_outputs(i):
    """Both sides are float64 sums over at most 1536 terms at magnitudes of about 10: another order moves them by about 1e-12.  Gate 1e-9."""
    c, a = GOLDEN[i]
    out = L.run_oracle_case(c)
    assert out.shape == (1, L.EMBED, c["h"], c["w"])
    assert np.abs(out[:, ::L.CHANNEL_STRIDE] - a["out64"]).max() <= 1e-9
    assert abs(np.abs(out).max() - a["max_abs"]) <= 1e-9


def test_header_names_are_exactly_the_exported_symbols():
    hdr = open(os.path.join(ROOT, "include", "wg_dino.h")).read()
    names = {"wg_dino_scratch_floats", "wg_dino_features", "wg_dino_attention"}
    assert set(re.findall(r"\b(wg_dino_\w+)\s*\(", hdr)) == names
    blob = open(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so"), "rb").read()
    assert {n.decode() for n in re.findall(rb"(?<![A-Za-z0-9_])wg_dino_[a-z_]+", blob)} == names
    # the ctypes mirror and the header agree on the args block: 7 scalars' worth of head, 8 + 12 * 14 + 5 pointers, one int64
    assert C.sizeof(D.Block) == 14 * 8 and C.sizeof(D.Args) == 8 + 6 * 4 + 6 * 8 + 12 * 14 * 8 + 2 * 8 + 8 + 8 + 8 + 8
    for name, value in (("PATCH", D.PATCH), ("EMBED", D.EMBED), ("HEADS", D.HEADS), ("HEAD_DIM", D.HEAD_DIM), ("HIDDEN", D.HIDDEN),
                        ("LEAD_TOKENS", D.LEAD_TOKENS), ("MAX_BLOCKS", D.MAX_BLOCKS)):
        assert re.search(rf"#define WG_DINO_{name} {value}\b", hdr), name


def test_scratch_floats_is_the_documented_formula():
    f = D._lib.wg_dino_scratch_floats
    per_token = 384 + 384 + 1536
    for B, h, w in [(1, 1, 1), (2, 6, 10), (1, 86, 115), (1, 78, 138), (2, 19, 25), (1, 37, 37), (0, 3, 3), (1, 0, 7)]:
        assert f(B, h, w) == B * (5 + h * w) * per_token == D.scratch_floats(B, h, w), (B, h, w)
    assert f(-1, 1, 1) == BAD and f(1, -1, 1) == BAD and f(1, 1, -1) == BAD
    assert f(1, 40000, 40000) < 0 and f(2, 700, 700) < 0      # the count leaves 31 bits
    with pytest.raises(RuntimeError):
        D.scratch_floats(1, -2, 3)


def _args(**over):
    """A well-formed args block on fake device addresses (never dereferenced: every call made with it is refused on its arguments)."""
    p = 4096
    a = D.Args()
    a.struct_size = C.sizeof(D.Args)
    a.B, a.H, a.W, a.num_blocks, a.eps = 1, 28, 42, 6, 1e-6
    for name in ("image", "patch_w", "patch_b", "pos", "cls_token", "reg_tokens", "norm_w", "norm_b", "scratch", "out"):
        setattr(a, name, p)
    for i in range(D.MAX_BLOCKS):
        for name in D.BLOCK_FIELDS:
            setattr(a.blocks[i], name, p)
    a.scratch_floats = D.scratch_floats(1, 2, 3)
    for k, v in over.items():
        if k.startswith("block_"):
            setattr(a.blocks[3], k[len("block_"):], v)
        else:
            setattr(a, k, v)
    return a


def test_malformed_calls_are_refused_before_any_device_work():
    f = lambda **over: D._lib.wg_dino_features(C.byref(_args(**over)))
    assert D._lib.wg_dino_features(None) == BAD
    assert f(struct_size=C.sizeof(D.Args) - 8) == BAD and f(struct_size=0) == BAD
    for name in ("image", "patch_w", "patch_b", "pos", "cls_token", "reg_tokens", "norm_w", "norm_b", "scratch", "out"):
        assert f(**{name: None}) == BAD, name
    for name in D.BLOCK_FIELDS:   # a block that is run ...
        assert f(**{"block_" + name: None}) == BAD, name
    for H, W in [(0, 42), (28, 0), (-14, 42), (28, -42), (27, 42), (28, 43), (29, 42), (13, 14), (14, 15)]:
        assert f(H=H, W=W) == BAD, (H, W)
    for n in (0, -1, 13, 100):
        assert f(num_blocks=n) == BAD, n
    assert f(B=0) == BAD and f(B=-1) == BAD
    assert f(eps=0.0) == BAD and f(eps=-1e-6) == BAD
    assert f(gemm_tiling=3) == BAD and f(gemm_tiling=-1) == BAD
    assert f(scratch_floats=D.scratch_floats(1, 2, 3) - 1) == BAD
    assert f(H=14 * 1000, W=14 * 1000, scratch_floats=2**62) == BAD   # index arithmetic would leave 31 bits
    p = C.c_void_p(4096)
    att = D._lib.wg_dino_attention
    assert att(None, 1, 6, p, None) == BAD and att(p, 1, 6, None, None) == BAD
    assert att(p, 0, 6, p, None) == BAD and att(p, 1, 0, p, None) == BAD and att(p, -1, 6, p, None) == BAD and att(p, 1, -6, p, None) == BAD
    assert att(p, 1, 2**31 - 1, p, None) == BAD


def test_structure_coverage_is_decided_on_the_module_alone():
    bb = L.TorchBackbone()
    assert D.structure_covered(bb) and D.structure_covered(bb, 0) and D.structure_covered(bb, 11)
    assert not D.structure_covered(bb, 12) and not D.structure_covered(bb, -1)
    assert not D.model_covered(bb)                                # CPU parameters
    x = torch.zeros(1, 3, 28, 42)
    assert not D.DinoFeatures.covers(bb, x) and not D.DinoFeatures.covers(None, x)
    with pytest.raises(RuntimeError):
        D.DinoFeatures(bb)                                         # there is no CPU path
    bb.chunked_blocks = True
    assert not D.structure_covered(bb)
    bb.chunked_blocks = False
    bb.blocks[3].mlp.act = torch.nn.GELU(approximate="tanh")
    assert not D.structure_covered(bb) and D.structure_covered(bb, 2)          # only the blocks that are run are looked at
    bb.blocks[1].mlp.fc1 = torch.nn.Linear(L.EMBED, 1024)
    assert not D.structure_covered(bb, 2)
    assert not D.structure_covered(types.SimpleNamespace(patch_size=14, num_heads=6))
    other = L.TorchBackbone()
    other.register_tokens = None
    assert not D.structure_covered(other)


def test_position_embedding_takes_both_branches_of_the_model():
    bb = L.TorchBackbone(L.make_weights())
    pe = bb.pos_embed.detach()
    assert torch.equal(D.prepare_pos_embed(bb, 37, 37), pe[0])                                    # as it is
    assert torch.equal(D.prepare_pos_embed(bb, 5, 7), L.pos_embed_for(pe, 5, 7, 0.0, True))
    bb.interpolate_offset, bb.interpolate_antialias = 0.1, False
    other = D.prepare_pos_embed(bb, 5, 7)
    assert torch.equal(other, L.pos_embed_for(pe, 5, 7, 0.1, False)) and not torch.equal(other, L.pos_embed_for(pe, 5, 7, 0.0, True))
    assert tuple(other.shape) == (36, L.EMBED)


class _FakeExtractor:
    """Stands in for wg_fused_dino.DinoFeatures: covers float32 [B, 3, H, W] with H, W multiples of 14; features are a function of the input."""
    made = 0

    def __init__(self, backbone, block=None):
        type(self).made += 1
        self.backbone, self.calls = backbone, 0

    @staticmethod
    def covers(backbone, x, block=None, masks=None):
        return backbone is not None and torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] % 14 == 0 and x.shape[3] % 14 == 0

    def input_covered(self, x, masks=None):
        return _FakeExtractor.covers(self.backbone, x, masks=masks)

    def features(self, x):
        self.calls += 1
        return x.mean() + torch.zeros(x.shape[0], 8, x.shape[2] // 14, x.shape[3] // 14)


def _stub_module():
    m = types.ModuleType("stub_method")
    m.GaussianModel = type("GaussianModel", (), {})

    class UncertaintyModel:
        def __init__(self):
            self.backbone, self._images_cache, self.original_calls = object(), {}, []

        def _get_dino_cached(self, x, cache_entry=None):
            self.original_calls.append((tuple(x.shape), cache_entry))
            return "original"
    m.UncertaintyModel = UncertaintyModel
    return m


def test_wrapper_keeps_the_callers_cache_and_serves_only_covered_calls(monkeypatch):
    import inspect
    import wg_integration
    params = inspect.signature(wg_integration.apply_optins).parameters
    assert params["uncertainty_backbone"].default is False and params["uncertainty_feature_cache"].default is False
    monkeypatch.setattr(D, "DinoFeatures", _FakeExtractor)
    _FakeExtractor.made = 0
    m = _stub_module()
    orig = m.UncertaintyModel._get_dino_cached
    undo = wg_integration.apply_optins(m, **OTHERS_OFF)
    assert m.UncertaintyModel._get_dino_cached is orig            # off by default
    undo()
    with pytest.raises(ValueError):
        wg_integration.apply_optins(m, uncertainty_feature_cache=True, **OTHERS_OFF)
    assert m.UncertaintyModel._get_dino_cached is orig

    undo = wg_integration.apply_optins(m, uncertainty_backbone=True, **OTHERS_OFF)
    assert m.UncertaintyModel._get_dino_cached is not orig
    model = m.UncertaintyModel()
    x = torch.rand(1, 3, 28, 42)
    # no cache entry: computed, nothing stored
    f0 = model._get_dino_cached(x)
    assert tuple(f0.shape) == (1, 8, 2, 3) and model._images_cache == {} and _FakeExtractor.made == 1
    # an entry: stored under the shape of the FEATURES, as a detached CPU tensor with the same values
    f1 = model._get_dino_cached(x, "frame7")
    assert list(model._images_cache) == [("frame7", f1.shape)] and torch.equal(model._images_cache[("frame7", f1.shape)], f1)
    # ... and the look-up, under the shape of the INPUT, never hits: the second visit computes again, as on the unchanged caller
    ex = model.__dict__["_wg_dino_features"]
    model._get_dino_cached(x, "frame7")
    assert ex.calls == 3 and _FakeExtractor.made == 1 and len(model._images_cache) == 1
    # a key that does hit is served from the cache, moved to the input's device
    model._images_cache[("hit", x.shape)] = torch.full((1, 8, 2, 3), 5.0)
    assert torch.equal(model._get_dino_cached(x, "hit"), torch.full((1, 8, 2, 3), 5.0)) and ex.calls == 3
    # uncovered calls reach the original method with the caller's arguments
    assert model._get_dino_cached(x.double(), "e") == "original" and model._get_dino_cached(torch.rand(1, 3, 27, 42)) == "original"
    assert model.original_calls == [((1, 3, 28, 42), "e"), ((1, 3, 27, 42), None)]
    # another backbone object on the model: a new extractor
    model.backbone = object()
    model._get_dino_cached(x)
    assert _FakeExtractor.made == 2
    undo()
    assert m.UncertaintyModel._get_dino_cached is orig


def test_feature_cache_registers_the_same_tensor_under_the_key_that_is_looked_up(monkeypatch):
    import wg_integration
    monkeypatch.setattr(D, "DinoFeatures", _FakeExtractor)
    m = _stub_module()
    orig = m.UncertaintyModel._get_dino_cached
    undo = wg_integration.apply_optins(m, uncertainty_backbone=True, uncertainty_feature_cache=True, **OTHERS_OFF)
    model = m.UncertaintyModel()
    x = torch.rand(1, 3, 28, 42)
    f1 = model._get_dino_cached(x, "frame7")
    ex = model.__dict__["_wg_dino_features"]
    assert set(model._images_cache) == {("frame7", f1.shape), ("frame7", x.shape)}
    assert model._images_cache[("frame7", f1.shape)] is model._images_cache[("frame7", x.shape)]      # no second copy
    f2 = model._get_dino_cached(x, "frame7")
    assert ex.calls == 1 and torch.equal(f1, f2)                   # the second visit makes no backbone call
    model._get_dino_cached(torch.rand(1, 3, 14, 14), "frame7")     # another input shape of the same frame is another entry
    assert ex.calls == 2 and len(model._images_cache) == 4
    model._get_dino_cached(x)                                      # no entry named: never cached
    assert ex.calls == 3 and len(model._images_cache) == 4
    undo()
    assert m.UncertaintyModel._get_dino_cached is orig


def test_the_new_switches_are_documented():
    for doc in ("docs/OPTIONS.md", "INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "uncertainty_backbone" in text and "uncertainty_feature_cache" in text, doc
    assert "dino/vit.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---------------------------------------------------------------- GPU

def _device():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _backbone(peaked=False, offset=0.0, antialias=True):
    return L.TorchBackbone(L.make_weights(peaked), offset=offset, antialias=antialias).to(_device())


@functools.lru_cache(maxsize=None)
def _extractor(peaked=False, offset=0.0, antialias=True, block=L.HEADS - 1):
    return D.DinoFeatures(_backbone(peaked, offset, antialias), block=block)


@functools.lru_cache(maxsize=None)
def _run(i):
    """Case i through the fused extractor, twice, and through the float64 oracle.  Computed once, shared by the tests below, never modified."""
    c, _ = GOLDEN[i]
    ex = _extractor(c["peaked"], c["offset"], c["antialias"], c["block"])
    x = L.make_image(c).to(_device())
    got, again = ex.features(x).cpu().numpy(), ex.features(x).cpu().numpy()
    return got, again, L.run_oracle_case(c)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_state_behind():
    """The backbones, extractors and results the GPU tests share live in the caches above; they are dropped when this module is done, so that
    the tests that follow it in the same process find the device allocator as this module found it (no empty_cache: that would also drop
    what earlier modules left cached)."""
    yield
    for cached in (_run, _extractor, _backbone):
        cached.cache_clear()
    gc.collect()


def _record(case, entry):
    if not os.environ.get("WG_RECORD"):
        return
    path = os.path.join(ROOT, "profiles", "dino_backbone", "accuracy.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {
        "metric": "dino_backbone_accuracy", "yardstick": "max |fused - float64 oracle| over the whole tensor / max(ref32_dev, 16 float32 ulps of the "
        "output's largest magnitude); ref32_dev = the reference's own max |float32 - float64| on the same input (tests/golden/dino_ref.npz); the "
        "gate (tests/test_dino_backbone.py) is 4", "device": torch.cuda.get_device_name(0), "cases": {}}
    data["cases"][case] = entry
    data["largest"] = max(e["ratio"] for e in data["cases"].values())
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_features_are_within_four_times_the_reference_float32_error(i):
    c, a = GOLDEN[i]
    got, _, ref = _run(i)
    assert got.dtype == np.float32 and got.shape == ref.shape == (1, L.EMBED, c["h"], c["w"]) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    unit = max(a["ref32_dev"], ULP16(a["max_abs"]))
    print(f"{c['name']}: max|fused - f64| = {err:.3e}, ref32_dev = {a['ref32_dev']:.3e}, floor = {ULP16(a['max_abs']):.3e}, ratio = {err / unit:.3f} (gate 4)")
    _record(c["name"], {"max_err": float(err), "ref32_dev": a["ref32_dev"], "ratio": float(err / unit)})
    assert err <= gate(a["ref32_dev"], a["max_abs"])


@pytest.mark.gpu
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_two_calls_give_identical_bits(i):
    got, again, _ = _run(i)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def _qkv(B, N, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((B, N, 3, L.HEADS, L.HEAD_DIM)).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [1, 6, 63, 64, 65, 127, 128, 129, 255, 257, 1000])
def test_attention_alone_against_the_float64_softmax(N, B):
    qkv = _qkv(B, N, 100 * N + B)
    ref = L.attention64(qkv).numpy()
    dev32 = np.abs(L.attention32_reference_formula(qkv).double().numpy() - ref).max()
    got = D.attention(qkv.to(_device())).cpu().numpy()
    assert got.shape == (B, N, L.EMBED) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"N = {N}, B = {B}: max|fused - f64| = {err:.3e}, float32 formula {dev32:.3e}, floor {ULP16(np.abs(ref).max()):.3e}")
    assert err <= gate(dev32, np.abs(ref).max())
    if B == 2:   # image b of a batch is the single call, bit for bit
        for b in range(B):
            assert torch.equal(D.attention(qkv[b:b + 1].to(_device())).cpu()[0], torch.from_numpy(got[b]))


@pytest.mark.gpu
def test_attention_with_one_dominant_key_per_row_returns_that_keys_value():
    """N = 65: q_i = 64 e_(i mod 64), k_j = 4 e_j for j < 64 and k_64 = 0: row i scores 32 at key i mod 64 and 0 elsewhere, in every head."""
    N = 65
    qkv = 0.0 * _qkv(1, N, 5)
    qkv[0, :, 2] = _qkv(1, N, 6)[0, :, 2]
    for i in range(N):
        qkv[0, i, 0, :, i % 64] = 64.0
        if i < 64:
            qkv[0, i, 1, :, i] = 4.0
    ref = L.attention64(qkv).numpy()
    dev32 = np.abs(L.attention32_reference_formula(qkv).double().numpy() - ref).max()
    got = D.attention(qkv.to(_device())).cpu().numpy().astype(np.float64)
    want = qkv[0, [i % 64 for i in range(N)], 2].reshape(N, L.EMBED).double().numpy()
    bound = gate(dev32, np.abs(ref).max())
    assert np.abs(ref[0] - want).max() <= 1e-10                   # the construction does what it says
    assert np.abs(got[0] - want).max() <= bound and np.abs(got - ref).max() <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 129])
def test_attention_ignores_nan_behind_the_last_token(N):
    """Keys and values past N, in the slack a caller's buffer may have, are never part of a result: the ragged last tile is masked."""
    dev = _device()
    slack, guard = 70, 64
    clean = _qkv(1, N, 40 + N).to(dev)
    padded = torch.full((N + slack, 3 * L.EMBED), float("nan"), device=dev)
    padded[:N] = clean.reshape(N, -1)
    out = torch.full((guard + (N + slack) * L.EMBED + guard,), 777.0, device=dev)
    D._native._check(D._lib.wg_dino_attention(padded.data_ptr(), 1, N, out[guard:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                     "wg_dino_attention")
    got = out[guard:guard + N * L.EMBED].reshape(1, N, L.EMBED)
    assert torch.equal(got, D.attention(clean))
    assert bool((out[:guard] == 777.0).all()) and bool((out[guard + N * L.EMBED:] == 777.0).all())      # and no row past N is stored


@pytest.mark.gpu
def test_a_batch_of_two_images_equals_the_two_single_calls_bit_for_bit():
    c, _ = GOLDEN[IDS.index("6x10")]
    ex = _extractor()
    x = L.make_image(c, B=2).to(_device())
    assert not torch.equal(x[0], x[1])
    both = ex.features(x)
    assert tuple(both.shape) == (2, L.EMBED, c["h"], c["w"])
    for b in range(2):
        assert torch.equal(both[b], ex.features(x[b:b + 1])[0])
    assert not torch.equal(both[0], both[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "4x31", "37x37"])
def test_both_gemm_tilings_give_the_bits_of_the_automatic_choice(name):
    """The 128 x 128 tiling runs where it has at least 128 workgroups (at 37 x 37: FC1 alone; the threshold's other side for the rest), the
    64 x 64 one elsewhere; each output element is the same k-ordered chain in both, so forcing either must change no bit.  129 tokens: a
    ragged second 128-row tile and a ragged third 64-row tile."""
    i = IDS.index(name)
    c, _ = GOLDEN[i]
    ex = _extractor()
    x = L.make_image(c).to(_device())
    auto = torch.from_numpy(_run(i)[0]).to(_device())
    assert torch.equal(ex.features(x, _gemm_tiling=1), auto) and torch.equal(ex.features(x, _gemm_tiling=2), auto)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "6x10", "12x21"])
def test_guard_floats_around_output_and_scratch_are_untouched(name):
    c, _ = GOLDEN[IDS.index(name)]
    ex = _extractor()
    x = L.make_image(c, B=2).to(_device())
    g = 64
    for tiling in (1, 2):
        out, out_buf, scratch = ex.features(x, _guard_floats=g, _gemm_tiling=tiling)
        assert torch.equal(out, ex.features(x))
        for buf in (out_buf, scratch):
            assert bool((buf[:g] == 12345.0).all()) and bool((buf[-g:] == 12345.0).all())
    assert scratch.numel() == D.scratch_floats(2, c["h"], c["w"]) + 2 * g


@pytest.mark.gpu
def test_weights_are_repacked_after_an_in_place_change_and_after_load_state_dict():
    c, _ = GOLDEN[IDS.index("6x10")]
    bb = L.TorchBackbone(L.make_weights()).to(_device())
    ex = D.DinoFeatures(bb)
    x = L.make_image(c).to(_device())
    first = ex.features(x).clone()
    old = {k: v.clone() for k, v in bb.state_dict().items()}
    with torch.no_grad():
        bb.blocks[4].mlp.fc2.weight.mul_(1.25)                    # in place: the version counter moves, the storage stays
    changed = ex.features(x).clone()
    assert not torch.equal(changed, first)
    with torch.no_grad():
        bb.blocks[9].mlp.fc2.weight.mul_(1.25)                    # a block that is not run: no output changes
    assert torch.equal(ex.features(x), changed)
    bb.load_state_dict(old)
    assert torch.equal(ex.features(x), first)
    with torch.no_grad():
        bb.norm.bias.data = bb.norm.bias.data + 1.0               # a new storage under the same parameter
    assert not torch.equal(ex.features(x), first)


def _method_stub(model_class):
    m = types.ModuleType("stub_method")
    m.GaussianModel = type("GaussianModel", (), {})
    m.UncertaintyModel = model_class
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("with_loss", [False, True], ids=["backbone-only", "with-uncertainty-loss"])
def test_the_opt_in_keeps_get_dino_cached_within_the_gate_of_the_unswapped_call(with_loss):
    import uncertainty_lib as U
    import wg_integration
    dev = _device()
    c, a = GOLDEN[IDS.index("6x10")]
    bb = L.TorchBackbone(L.make_weights()).to(dev)
    model, Model = L.stand_in_uncertainty_model(bb)
    model = model.to(dev)
    original = Model.__dict__.get("_get_dino_cached", None)
    x = L.make_image(c).to(dev)
    ref = L.run_oracle_case(c)
    bound = gate(a["ref32_dev"], a["max_abs"])
    plain = model._get_dino_cached(x, "frame")
    plain_cache = dict(model._images_cache)
    assert bb.calls == 1 and np.abs(plain.cpu().double().numpy() - ref).max() <= bound
    model._images_cache.clear()
    undo = wg_integration.apply_optins(_method_stub(Model), uncertainty_backbone=True, uncertainty_loss=with_loss, **OTHERS_OFF)
    try:
        fused = model._get_dino_cached(x, "frame")
        assert bb.calls == 1                                       # the torch backbone was not called again
        assert fused.shape == plain.shape and fused.device == plain.device and fused.dtype == plain.dtype
        assert np.abs(fused.cpu().double().numpy() - ref).max() <= bound
        assert np.abs((fused - plain).cpu().double().numpy()).max() <= 2 * bound
        # the cache: the caller's keys and shapes, CPU tensors holding what was returned
        assert list(model._images_cache) == list(plain_cache) == [("frame", plain.shape)]
        stored = model._images_cache[("frame", plain.shape)]
        assert not stored.is_cuda and torch.equal(stored, fused.cpu())
        ragged = torch.rand(1, 3, 30, 42, device=dev)             # a height that is no multiple of 14: uncovered, the caller's own method
        assert tuple(model._get_dino_cached(ragged, "other").shape) == (1, L.EMBED, 2, 3) and bb.calls == 2
        if with_loss:   # compute_losses reaches the backbone through the swapped method: three fused calls, none of torch's
            gt, pred = U.make_images({"H": 60, "W": 85, "seed": 4100})
            loss, metrics, loss_mult = model._compute_losses(gt.to(dev), pred.to(dev), "train/", _cache_entry="frame60")
            assert bb.calls == 2 and torch.isfinite(loss) and tuple(loss_mult.shape) == (1, 1, 60, 85) and "train/psnr_discounted" in metrics
    finally:
        undo()
    assert Model._get_dino_cached is U.StandInModel._get_dino_cached or Model.__dict__.get("_get_dino_cached") is original
    assert model._get_dino_cached(x).shape == plain.shape and bb.calls == 3   # undone: the torch backbone again
