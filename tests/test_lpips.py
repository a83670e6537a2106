"""Fused LPIPS v0.1 on the AlexNet and VGG16 trunks (include/wg_lpips.h, wg_fused_lpips, wg_integration.fuse_evaluation_lpips) against the
reference's `LPIPS.forward` (wildgaussians/_metrics_lpips.py:149-180) as `evaluation._lpips` (wildgaussians/evaluation.py:255-291) feeds it.

Oracle: tests/lpips_lib.py's float64 restatement, pinned (on the CPU) to the float64 values and taps recorded from the reference's own class in
tests/golden/lpips_ref.npz.  Weights and images are regenerated from seeds.
Gate, the project's own: |fused - float64| <= 4 * max(ref32_dev, floor), ref32_dev = the reference's recorded |float32 - float64| of the same
quantity on the same input, floor = 16 float32 ulps of the quantity's largest magnitude.  Applied element-wise to every tap tensor (both
images), to each layer value and to the total.  For the scalars the floor governs: the reference's float32 run is 6e-9 to 1e-7 away from its
float64 run on totals of about 1.  The convolution stage alone is held the same way against float64 conv2d, ref32_dev being float32 conv2d's
error on the CPU.
Cases (tests/lpips_lib.CASES): alex 31x31 (the minimum), 32x35, 35x67, 64x48, 97x130, 131x259; vgg 16x16 (the minimum), 17x33, 31x47, 50x70,
64x96; batches of 2 and 3 at alex 31x31 and vgg 17x33.
Measured on an MI355X (profiles/lpips/accuracy.json), as ratios of max(ref32_dev, floor) against the gate of 4: tap elements at most 2.09
(vgg 31x47, tap 4), layer values at most 2.22 (vgg 17x33 B = 3, layer 4: 1 x 2 pixels of 512 channels), totals at most 0.044."""
import ctypes as C
import functools
import gc
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wild-gaussians_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_lib as L  # noqa: E402
import wg_fused_lpips as D  # noqa: E402

GOLDEN = L.load_golden()
IDS = [L.case_id(c) for c, _ in GOLDEN]
INDEX = list(range(len(GOLDEN)))
ULP16 = lambda largest: 16 * float(np.spacing(np.float32(largest)))
BAD, OVERFLOW = -1, -4   # WG_ERR_INVALID_ARGUMENT, WG_ERR_OVERFLOW
NET = {"alex": D.ALEX, "vgg": D.VGG}


def gate(ref32_dev, largest):
    return 4 * max(float(ref32_dev), ULP16(largest))


# ---------------------------------------------------------------- CPU: the fixture, the oracle, the C-ABI, the opt-in's logic

def test_fixture_holds_the_cases_of_the_issue_and_stays_small():
    sizes = {(c["net"], c["H"], c["W"], c["B"]) for c, _ in GOLDEN}
    assert {("alex", 31, 31, 1), ("alex", 32, 35, 1), ("alex", 35, 67, 1), ("alex", 64, 48, 1), ("alex", 97, 130, 1), ("alex", 131, 259, 1),
            ("vgg", 16, 16, 1), ("vgg", 17, 33, 1), ("vgg", 31, 47, 1), ("vgg", 50, 70, 1), ("vgg", 64, 96, 1),
            ("alex", 31, 31, 2), ("alex", 31, 31, 3), ("vgg", 17, 33, 2), ("vgg", 17, 33, 3)} == sizes
    for c, a in GOLDEN:
        assert a["total64"].dtype == np.float64 and a["total64"].shape == (c["B"],) and a["layers64"].shape == (c["B"], L.TAPS)
        assert 0.1 <= a["total64"].min() and a["total64"].max() <= 2.0 and a["total32_dev"].max() < 1e-6
        for l, cn in enumerate(L.CHANNELS[c["net"]]):
            assert a[f"tap{l}_64"].dtype == np.float64 and a[f"tap{l}_64"].shape[:2] == (c["B"], cn // L.CHANNEL_STRIDE)
            assert 0 < a[f"tap{l}_ref32_dev"] < 1e-4 and 0.1 < a[f"tap{l}_max_abs"] < 100
    assert os.path.getsize(L.GOLDEN) < 1_000_000


@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_float64_oracle_reproduces_the_recorded_reference_outputs(i):
    c, a = GOLDEN[i]
    total, layers, t0, t1 = L.run_oracle_case(c["name"])
    assert np.abs(total - a["total64"]).max() <= 1e-12 and np.abs(layers - a["layers64"]).max() <= 1e-12
    for l in range(L.TAPS):
        assert t0[l].shape[1] == L.CHANNELS[c["net"]][l]
        assert np.abs(t0[l][:, ::L.CHANNEL_STRIDE] - a[f"tap{l}_64"]).max() <= 1e-12
        assert abs(max(np.abs(t0[l]).max(), np.abs(t1[l]).max()) - a[f"tap{l}_max_abs"]) <= 1e-12


def test_stand_in_module_is_the_oracle_in_float32():
    c, a = GOLDEN[IDS.index("alex-32x35")]
    pred, gt = L.make_images(c)
    m = L.StandInLPIPS("alex", L.make_weights("alex"))
    with torch.no_grad():
        val, res = m(pred.clamp(0, 1) * 2 - 1, gt.clamp(0, 1) * 2 - 1, retPerLayer=True)
    assert tuple(val.shape) == (1, 1, 1, 1) and len(res) == L.TAPS
    assert abs(float(val) - a["total64"][0]) <= 4 * max(a["total32_dev"][0], ULP16(a["total64"][0]))


def test_header_names_are_exactly_the_exported_symbols():
    hdr = open(os.path.join(ROOT, "include", "wg_lpips.h")).read()
    names = {"wg_lpips", "wg_lpips_scratch_floats", "wg_lpips_conv", "wg_lpips_pool", "wg_lpips_head"}
    assert set(re.findall(r"\b(wg_lpips\w*)\s*\(", hdr)) == names
    blob = open(os.path.join(ROOT, "wild-gaussians_amd", "diff_gaussian_rasterization", "libwg_rasterizer.so"), "rb").read()
    assert {n.decode() for n in re.findall(rb"(?<![A-Za-z0-9_])wg_lpips[a-z_]*(?![A-Za-z0-9_.])", blob)} == names
    for name, value in (("ALEX", D.ALEX), ("VGG", D.VGG), ("TAPS", D.TAPS), ("MAX_CONVS", D.MAX_CONVS), ("HEAD_PIXELS", D.HEAD_PIXELS),
                        ("ALEX_MIN_SIDE", D.MIN_SIDE[D.ALEX]), ("VGG_MIN_SIDE", D.MIN_SIDE[D.VGG])):
        assert re.search(rf"#define WG_LPIPS_{name} {value}\b", hdr), name
    # the ctypes mirrors and the header agree: 8 + 4 x 4 bytes of head, two images of 5 x 8, 2 + 13 + 13 + 5 + 1 pointers, an int64, 3 pointers
    assert C.sizeof(D.Image) == 40 and C.sizeof(D.Args) == 8 + 16 + 2 * 40 + (2 + 13 + 13 + 5 + 1) * 8 + 8 + 3 * 8
    assert C.sizeof(D.ConvArgs) == 8 + 8 * 4 + 8 + 2 * 40 + 8 + 6 * 8
    assert "lpips/lpips.hip" in open(os.path.join(ROOT, "wild-gaussians_amd", "build.py")).read()


def _documented_scratch(net, B, H, W):
    chunks = lambda n: (n + 255) // 256
    if net == D.VGG:
        sizes, h, w = [], H, W
        for _ in range(5):
            sizes.append((h, w))
            h, w = h // 2, w // 2
        A = 2 * B * 64 * H * W
    else:
        h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
        h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
        h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
        sizes = [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]
        A = 2 * B * 64 * h1 * w1
    return 2 * A + 2 * B * sum(chunks(h * w) for h, w in sizes)


def test_scratch_floats_is_the_documented_formula():
    f = D._lib.wg_lpips_scratch_floats
    for net, B, H, W in [(D.ALEX, 1, 31, 31), (D.ALEX, 3, 131, 259), (D.ALEX, 1, 1200, 1600), (D.VGG, 1, 16, 16), (D.VGG, 2, 17, 33),
                         (D.VGG, 1, 1200, 1600), (D.VGG, 1, 1080, 1920)]:
        assert f(net, B, H, W) == _documented_scratch(net, B, H, W) == D.scratch_floats(net, B, H, W), (net, B, H, W)
    assert f(D.VGG, 1, 1200, 1600) * 4 == pytest.approx(1.97e9, rel=0.01)
    assert f(2, 1, 64, 64) == BAD and f(-1, 1, 64, 64) == BAD and f(D.ALEX, 0, 64, 64) == BAD and f(D.VGG, -1, 64, 64) == BAD
    assert f(D.ALEX, 1, 30, 64) == BAD and f(D.ALEX, 1, 64, 30) == BAD and f(D.VGG, 1, 15, 64) == BAD and f(D.VGG, 1, 64, 15) == BAD
    assert f(D.VGG, 1, 5000, 5000) == OVERFLOW and f(D.VGG, 16, 1200, 1600) == OVERFLOW and f(D.ALEX, 1, 40000, 40000) == OVERFLOW
    with pytest.raises(RuntimeError):
        D.scratch_floats(D.VGG, 1, 8, 8)


def _args(**over):
    """A well-formed args block on fake device addresses (never dereferenced: every call made with it is refused on its arguments)."""
    p = 4096
    a = D.Args()
    a.struct_size, a.net, a.B, a.H, a.W = C.sizeof(D.Args), D.ALEX, 1, 40, 50
    a.in0 = D.Image(p, 6000, 50, 1, 2000)
    a.in1 = D.Image(p, 6000, 150, 3, 1)
    for name in ("shift", "scale", "scratch", "out", "per_layer"):
        setattr(a, name, p)
    for i in range(D.MAX_CONVS):
        a.conv_w[i], a.conv_b[i] = p, p
    for i in range(D.TAPS):
        a.lin_w[i] = p
    a.scratch_floats = D.scratch_floats(D.ALEX, 1, 40, 50)
    for k, v in over.items():
        if k in ("conv_w", "conv_b", "lin_w"):
            getattr(a, k)[v] = None
        else:
            setattr(a, k, v)
    return a


def test_malformed_calls_are_refused_before_any_device_work():
    f = lambda **over: D._lib.wg_lpips(C.byref(_args(**over)))
    assert D._lib.wg_lpips(None) == BAD
    assert f(struct_size=C.sizeof(D.Args) - 8) == BAD and f(struct_size=0) == BAD
    for name in ("shift", "scale", "scratch", "out"):
        assert f(**{name: None}) == BAD, name
    assert f(in0=D.Image(None, 1, 1, 1, 1)) == BAD and f(in1=D.Image(None, 1, 1, 1, 1)) == BAD and f(in0=D.Image(4096, 1, -1, 1, 1)) == BAD
    for i in range(5):
        assert f(conv_w=i) == BAD and f(conv_b=i) == BAD and f(lin_w=i) == BAD, i
    assert f(net=2) == BAD and f(net=-1) == BAD
    assert f(H=30) == BAD and f(W=30) == BAD and f(net=D.VGG, H=15, scratch_floats=2**40) == BAD and f(H=0) == BAD and f(W=-40) == BAD
    assert f(B=0) == BAD and f(B=-1) == BAD
    assert f(scratch_floats=D.scratch_floats(D.ALEX, 1, 40, 50) - 1) == BAD and f(scratch=4100) == BAD
    assert f(net=D.VGG, H=5000, W=5000, scratch_floats=2**62) == BAD   # index arithmetic would leave 31 bits
    # the stages
    p = C.c_void_p(4096)

    def conv(**over):
        a = D.ConvArgs(struct_size=C.sizeof(D.ConvArgs), N=1, IH=8, IW=8, Cin=64, Cout=64, K=3, stride=1, pad=1, x=4096, w=4096, bias=4096, y=8192)
        for k, v in over.items():
            setattr(a, k, v)
        return D._lib.wg_lpips_conv(C.byref(a))
    assert D._lib.wg_lpips_conv(None) == BAD and conv(struct_size=8) == BAD
    for bad in (dict(Cin=32), dict(Cin=4), dict(Cin=65), dict(Cout=32), dict(Cout=96), dict(Cout=0), dict(K=0), dict(K=12), dict(stride=0),
                dict(pad=-1), dict(pad=3), dict(N=0), dict(IH=0), dict(IW=-1), dict(w=None), dict(bias=None), dict(y=None), dict(w=4100),
                dict(x=None), dict(x=None, Cin=3), dict(IH=40000, IW=40000), dict(K=5, pad=0, IH=4)):
        assert conv(**bad) == BAD, bad
    pool = D._lib.wg_lpips_pool
    assert pool(None, 1, 8, 8, 64, 2, p, None) == BAD and pool(p, 1, 8, 8, 64, 2, None, None) == BAD and pool(p, 0, 8, 8, 64, 2, p, None) == BAD
    assert pool(p, 1, 8, 8, 64, 4, p, None) == BAD and pool(p, 1, 8, 8, 6, 2, p, None) == BAD and pool(p, 1, 2, 8, 64, 3, p, None) == BAD
    assert pool(p, 1, 40000, 40000, 64, 2, p, None) == BAD
    head = D._lib.wg_lpips_head
    assert head(None, 1, 4, 4, 64, p, p, p, None) == BAD and head(p, 1, 4, 4, 64, None, p, p, None) == BAD
    assert head(p, 1, 4, 4, 64, p, None, p, None) == BAD and head(p, 1, 4, 4, 64, p, p, None, None) == BAD
    assert head(p, 0, 4, 4, 64, p, p, p, None) == BAD and head(p, 1, 0, 4, 64, p, p, p, None) == BAD and head(p, 1, 4, 4, 32, p, p, p, None) == BAD
    assert head(p, 1, 4, 4, 576, p, p, p, None) == BAD and head(p, 1, 4, 4, 64, p, C.c_void_p(4100), p, None) == BAD
    assert head(p, 1, 40000, 40000, 64, p, p, p, None) == BAD


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_coverage_is_decided_on_the_module_alone(net):
    m = L.StandInLPIPS(net, L.make_weights(net))
    assert D.structure_covered(m)
    assert not D.structure_covered(None) and not D.structure_covered(torch.nn.Linear(3, 3))
    with pytest.raises(RuntimeError):
        D.LPIPS.from_module(torch.nn.Linear(3, 3))
    if net == "vgg":
        m.pnet_type = "vgg16"
        assert D.structure_covered(m)
    for change in (dict(pnet_type="squeeze"), dict(lpips=False), dict(spatial=True), dict(version="0.0")):
        other = L.StandInLPIPS(net, L.make_weights(net))
        for k, v in change.items():
            setattr(other, k, v)
        assert not D.structure_covered(other), change
    other = L.StandInLPIPS(net, L.make_weights(net))
    other.train()
    assert not D.structure_covered(other)
    other.eval()
    assert D.structure_covered(other)
    other.double()
    assert not D.structure_covered(other)
    other = L.StandInLPIPS(net)
    first = other.net.slice1[0]
    other.net.slice1[0] = torch.nn.Conv2d(3, 64, first.kernel_size, stride=first.stride, padding=0)
    assert not D.structure_covered(other)                 # another padding
    other = L.StandInLPIPS(net)
    other.net.slice3.add_module("extra", torch.nn.ReLU())
    assert not D.structure_covered(other)                 # another layer list
    other = L.StandInLPIPS(net)
    other.net.slice2[0] = torch.nn.MaxPool2d(3 if net == "alex" else 2, 2, ceil_mode=True)
    assert not D.structure_covered(other)
    other = L.StandInLPIPS(net)
    other.lins[2].model[1] = torch.nn.Conv2d(L.CHANNELS[net][2], 1, 1, bias=True)
    assert not D.structure_covered(other)
    assert not D.structure_covered(torch.nn.Module())


class _FakeFused:
    """Stands in for wg_fused_lpips.LPIPS: covers what the real one covers, on the CPU; the value is a function of the inputs."""
    made = 0

    def __init__(self, lp_net):
        type(self).made += 1
        self.module, self.net, self.device, self.calls, self.stale = lp_net, D.NET_OF[lp_net.pnet_type], torch.device("cpu"), [], False

    @classmethod
    def from_module(cls, lp_net, device=None):
        return cls(lp_net)

    def _fresh(self):
        if self.stale or self.module.training:
            raise RuntimeError("left the covered case")

    def input_covered(self, a, b):
        return a.shape == b.shape and a.dtype == torch.float32 and a.dim() == 4 and a.shape[1] == 3

    def __call__(self, a, b):
        self.calls.append((a, b))
        return (a - b).abs().mean((1, 2, 3))


def test_wrapper_routes_uncovered_calls_and_an_empty_cache_to_the_original(monkeypatch):
    import wg_integration
    assert list(inspect.signature(wg_integration.fuse_evaluation_lpips).parameters) == ["evaluation_module"]
    monkeypatch.setattr(D, "LPIPS", _FakeFused)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    _FakeFused.made = 0
    m = L.stand_in_evaluation_module(device="cpu")                 # the caller's own forward pass stays on the CPU
    original = m._lpips
    rng = np.random.default_rng(3)
    a, b = rng.random((2, 40, 36, 3)).astype(np.float32), rng.random((2, 40, 36, 3)).astype(np.float32)
    undo = wg_integration.fuse_evaluation_lpips(m)
    assert m._lpips is not original and m._lpips.__wrapped__ is original
    # an empty cache: the original builds and caches the network; nothing is constructed by the wrapper
    first = m.lpips(a, b)
    assert m.built == ["alex"] and len(m.original_calls) == 1 and m.original_calls[0][0] is a and m.original_calls[0][2] == "alex"
    assert _FakeFused.made == 0 and first.shape == (2,) and first.dtype == np.float32
    # from then on a covered call is served beside that cache entry: float32, reshaped to the batch shape
    got = m.lpips(a, b)
    assert len(m.original_calls) == 1 and _FakeFused.made == 1 and got.dtype == np.float32 and got.shape == (2,)
    assert np.allclose(got, np.abs(a - b).mean((1, 2, 3)), atol=1e-6)
    assert m.lpips(a[0], b[0]).shape == () and m.lpips(a[None], b[None]).shape == (1, 2) and _FakeFused.made == 1
    assert m.lpips(a.astype(np.float64), b.astype(np.float64)).dtype == np.float32
    assert m._lpips(a, b, "alex", "0.1").shape == (2,) and m._lpips(a=a, b=b, net="alex").shape == (2,) and len(m.original_calls) == 1
    # uncovered calls reach the original with the caller's arguments
    small = np.zeros((30, 36, 3), np.float32)
    with pytest.raises(RuntimeError):
        m.lpips(small, small)                                      # under the net's minimum: the caller's own pool refuses it
    m._lpips(a, b, "alex", version="0.0")                          # another version
    with pytest.raises(AssertionError):
        m.lpips(a, b[:1])                                          # shapes differ: the original's own assertion
    with pytest.raises(AssertionError):
        m.lpips((a * 255).astype(np.uint8), (b * 255).astype(np.uint8))
    four = np.zeros((40, 36, 4), np.float32)
    with pytest.raises(RuntimeError):
        m.lpips(four, four)                                        # four channels: the original's own convolution refuses them
    assert len(m.original_calls) == 6
    assert m.original_calls[1][0] is small and m.original_calls[2][3] == "0.0" and m.original_calls[3][1].shape == (1, 40, 36, 3)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m.lpips(a, b)                                                  # no HIP device
    assert len(m.original_calls) == 7
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    m.lpips_vgg(a, b)                                              # no vgg entry yet: the original builds it
    assert m.built == ["alex", "vgg"] and len(m.original_calls) == 8 and _FakeFused.made == 1
    m.lpips_vgg(a, b)
    assert _FakeFused.made == 2 and len(m.original_calls) == 8
    # a module that leaves the covered case; another object in the cache; an uncovered module
    m._LPIPS_CACHE["alex"].train()
    m.lpips(a, b)
    assert len(m.original_calls) == 9
    m._LPIPS_CACHE["alex"] = L.StandInLPIPS("alex", L.make_weights("alex"))
    m.lpips(a, b)
    assert _FakeFused.made == 3 and len(m.original_calls) == 9
    m._LPIPS_CACHE["alex"] = L.StandInLPIPS("alex", L.make_weights("alex"), spatial=True)
    m.lpips(a, b)
    m.lpips(a, b)
    assert _FakeFused.made == 3 and len(m.original_calls) == 11
    undo()
    assert m._lpips is original
    undo()                                                         # twice is harmless
    assert m._lpips is original


def test_undo_leaves_a_later_swap_alone():
    import wg_integration
    m = L.stand_in_evaluation_module()
    original = m._lpips
    undo = wg_integration.fuse_evaluation_lpips(m)
    other = lambda *a, **k: None
    m._lpips = other
    undo()
    assert m._lpips is other and original is not other


def test_the_switch_is_documented():
    import wg_integration
    assert "fuse_evaluation_lpips" in wg_integration.__doc__
    for doc in ("INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "fuse_evaluation_lpips" in text and "wg_fused_lpips" in text, doc
    assert "lpips/lpips.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---------------------------------------------------------------- GPU

def _device():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _module(net):
    return L.StandInLPIPS(net, L.make_weights(net)).to(_device())


@functools.lru_cache(maxsize=None)
def _fused(net):
    return D.LPIPS.from_module(_module(net))


@functools.lru_cache(maxsize=None)
def _run(i):
    """Case i through the fused operator, twice, with its taps.  Computed once, shared by the tests below, never modified."""
    c, _ = GOLDEN[i]
    op = _fused(c["net"])
    pred, gt = (t.to(_device()) for t in L.make_images(c))
    out, layers = op(pred, gt, per_layer=True)
    out2, layers2 = op(pred, gt, per_layer=True)
    taps0, taps1 = op.features(pred), op.features(gt)
    host = lambda t: t.cpu().numpy()
    return host(out), host(layers), host(out2), host(layers2), [host(t) for t in taps0], [host(t) for t in taps1]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_state_behind():
    """What the GPU tests share lives in the caches above; it is dropped when this module is done, so that the tests that follow in the same
    process find the device allocator as this module found it."""
    yield
    for cached in (_run, _fused, _module):
        cached.cache_clear()
    gc.collect()


def _record(case, entry):
    target = os.environ.get("WG_RECORD")
    if not target:
        return
    path = os.path.join(ROOT, "profiles", "lpips", "accuracy.json") if target == "1" else target
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {
        "metric": "lpips_accuracy", "yardstick": "max |fused - float64 oracle| / max(ref32_dev, 16 float32 ulps of the quantity's largest magnitude), "
        "element-wise over each tap tensor, for each layer value and for the total; ref32_dev = the reference's own |float32 - float64| on the same "
        "input (tests/golden/lpips_ref.npz); the gate (tests/test_lpips.py) is 4", "device": torch.cuda.get_device_name(0), "cases": {}}
    data["cases"].setdefault(case, {}).update(entry)
    data["largest"] = max(v for e in data["cases"].values() for v in e.values())
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_taps_are_within_four_times_the_reference_float32_error(i):
    c, a = GOLDEN[i]
    _, _, t0, t1 = L.run_oracle_case(c["name"])
    got0, got1 = _run(i)[4], _run(i)[5]
    ratios, failed = {}, []
    for l in range(L.TAPS):
        unit = max(float(a[f"tap{l}_ref32_dev"]), ULP16(a[f"tap{l}_max_abs"]))
        assert got0[l].dtype == np.float32 and got0[l].shape == t0[l].shape and got1[l].shape == t1[l].shape
        assert np.isfinite(got0[l]).all() and np.isfinite(got1[l]).all()
        err = max(np.abs(got0[l].astype(np.float64) - t0[l]).max(), np.abs(got1[l].astype(np.float64) - t1[l]).max())
        ratios[f"tap{l}"] = float(err / unit)
        print(f"{c['name']} tap {l} {t0[l].shape}: max|fused - f64| = {err:.3e}, ref32_dev = {a[f'tap{l}_ref32_dev']:.3e}, ratio = {err / unit:.3f} (gate 4)")
        if err > gate(a[f"tap{l}_ref32_dev"], a[f"tap{l}_max_abs"]):
            failed.append(l)
    _record(c["name"], ratios)
    assert not failed


@pytest.mark.gpu
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_layer_values_and_total_are_within_the_gate(i):
    c, a = GOLDEN[i]
    total, layers, _, _ = L.run_oracle_case(c["name"])
    out, lay = _run(i)[0], _run(i)[1]
    assert out.dtype == np.float32 and out.shape == (c["B"],) and lay.shape == (c["B"], L.TAPS) and np.isfinite(out).all() and np.isfinite(lay).all()
    ratios, failed = {}, []
    for b in range(c["B"]):
        for l in range(L.TAPS):
            err, unit = abs(float(lay[b, l]) - layers[b, l]), max(float(a["layers32_dev"][b, l]), ULP16(layers[b, l]))
            ratios[f"layer{l}"] = max(ratios.get(f"layer{l}", 0.0), float(err / unit))
            print(f"{c['name']} image {b} layer {l}: {lay[b, l]:.9g} against {layers[b, l]:.12g}: error {err:.3e}, ratio {err / unit:.3f} (gate 4)")
            if err > gate(a["layers32_dev"][b, l], layers[b, l]):
                failed.append((b, l))
        err, unit = abs(float(out[b]) - total[b]), max(float(a["total32_dev"][b]), ULP16(total[b]))
        ratios["total"] = max(ratios.get("total", 0.0), float(err / unit))
        print(f"{c['name']} image {b} total: {out[b]:.9g} against {total[b]:.12g}: error {err:.3e}, ratio {err / unit:.3f} (gate 4)")
        if err > gate(a["total32_dev"][b], total[b]):
            failed.append((b, "total"))
    _record(c["name"], ratios)
    assert not failed


@pytest.mark.gpu
@pytest.mark.parametrize("i", INDEX, ids=IDS)
def test_two_calls_give_identical_bits(i):
    out, lay, out2, lay2 = _run(i)[:4]
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(lay.view(np.uint32), lay2.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["alex-31x31-B2", "alex-31x31-B3", "vgg-17x33-B2", "vgg-17x33-B3"])
def test_a_batch_equals_the_single_calls_bit_for_bit(name):
    i = IDS.index(name)
    c, _ = GOLDEN[i]
    op = _fused(c["net"])
    pred, gt = (t.to(_device()) for t in L.make_images(c))
    out, lay = (torch.from_numpy(v).to(_device()) for v in _run(i)[:2])
    both = op.features(pred)
    for b in range(c["B"]):
        single, single_layers = op(pred[b], gt[b], per_layer=True)
        assert torch.equal(single, out[b:b + 1]) and torch.equal(single_layers, lay[b:b + 1])
        for tb, ts in zip(both, op.features(pred[b])):
            assert torch.equal(tb[b:b + 1], ts)
    assert len(set(out.tolist())) == c["B"]


@pytest.mark.gpu
@pytest.mark.parametrize("net,H,W", [("alex", 35, 67), ("vgg", 31, 47)])
def test_an_image_against_itself_is_exactly_zero(net, H, W):
    op = _fused(net)
    x = torch.rand(2, 3, H, W, device=_device())
    out, lay = op(x, x.clone(), per_layer=True)
    assert bool((out == 0).all()) and bool((lay == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["alex-31x31-B2", "alex-97x130", "vgg-17x33-B3", "vgg-31x47"])
def test_guard_floats_around_outputs_and_scratch_are_untouched(name):
    i = IDS.index(name)
    c, _ = GOLDEN[i]
    op = _fused(c["net"])
    pred, gt = (t.to(_device()) for t in L.make_images(c))
    g = 64
    out, lay, out_buf, lay_buf, scratch = op(pred, gt, per_layer=True, _guard_floats=g)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _run(i)[0].view(np.uint32))
    assert np.array_equal(lay.cpu().numpy().view(np.uint32), _run(i)[1].view(np.uint32))
    for buf in (out_buf, lay_buf, scratch):
        assert bool((buf[:g] == 12345.0).all()) and bool((buf[-g:] == 12345.0).all())
    assert scratch.numel() == D.scratch_floats(NET[c["net"]], c["B"], c["H"], c["W"]) + 2 * g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["alex-31x31-B2", "vgg-17x33-B2"])
def test_a_nan_in_image_0_leaves_image_1_unchanged(name):
    i = IDS.index(name)
    c, _ = GOLDEN[i]
    op = _fused(c["net"])
    pred, gt = (t.to(_device()) for t in L.make_images(c))
    pred = pred.clone()
    pred[0, 1, 9, 11] = float("nan")
    out, lay = op(pred, gt, per_layer=True)
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(lay[0, 0]))
    assert np.array_equal(out[1:].cpu().numpy().view(np.uint32), _run(i)[0][1:].view(np.uint32))
    assert np.array_equal(lay[1:].cpu().numpy().view(np.uint32), _run(i)[1][1:].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("net,H,W", [("alex", 35, 67), ("vgg", 17, 33)])
def test_first_layer_reads_any_strides_in_place_and_clips(net, H, W):
    dev = _device()
    op = _fused(net)
    rng = np.random.default_rng(H * W)
    raw = [torch.from_numpy(rng.uniform(-0.3, 1.3, (2, 3, H, W)).astype(np.float32)).to(dev) for _ in range(2)]
    planar = op(raw[0], raw[1], per_layer=True)
    hwc = [t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in raw]             # an uploaded H x W x 3 array
    assert hwc[0].stride() == (H * W * 3, 1, W * 3, 3)
    crops = []
    for t in raw:                                                                         # a window of a larger frame
        big = torch.full((2, 3, H + 5, W + 7), 0.5, device=dev)
        big[:, :, 2:2 + H, 3:3 + W] = t
        crops.append(big[:, :, 2:2 + H, 3:3 + W])
    assert not crops[0].is_contiguous()
    clipped = [t.clamp(0, 1) for t in raw]
    for other in (op(hwc[0], hwc[1], per_layer=True), op(crops[0], crops[1], per_layer=True), op(clipped[0], clipped[1], per_layer=True),
                  op(raw[0], hwc[1], per_layer=True)):
        assert torch.equal(other[0], planar[0]) and torch.equal(other[1], planar[1])
    for a, b in zip(op.features(raw[0]), op.features(crops[0])):
        assert torch.equal(a, b)
    assert not torch.equal(op(raw[0] * 0.5, raw[1])[0], planar[0])


@pytest.mark.gpu
def test_weights_are_repacked_after_an_in_place_change_and_after_load_state_dict():
    dev = _device()
    c, _ = GOLDEN[IDS.index("alex-35x67")]
    m = L.StandInLPIPS("alex", L.make_weights("alex")).to(dev)
    op = D.LPIPS.from_module(m)
    pred, gt = (t.to(dev) for t in L.make_images(c))
    first = op(pred, gt).clone()
    old = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        m.net.slice3[1].weight.mul_(1.25)                              # in place: the version counter moves, the storage stays
    changed = op(pred, gt).clone()
    assert not torch.equal(changed, first)
    with torch.no_grad():
        m.lins[0].model[1].weight.mul_(0.5)
    assert not torch.equal(op(pred, gt), changed)
    m.load_state_dict(old)
    assert torch.equal(op(pred, gt), first)
    m.train()
    with pytest.raises(RuntimeError):
        op(pred, gt)
    m.eval()
    assert torch.equal(op(pred, gt), first)
    cpu = D.LPIPS.from_module(L.StandInLPIPS("alex", L.make_weights("alex")), device=dev)   # a module that lives on the CPU
    assert torch.equal(cpu(pred, gt), first)
    with pytest.raises(RuntimeError):
        op(pred.cpu(), gt.cpu())                                   # there is no CPU path
    with pytest.raises(RuntimeError):
        op(pred[:, :, :30], gt[:, :, :30])


# (N, IH, IW, Cin, Cout, K, stride, pad): output pixel counts M of 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257 and a batch of two first layers
CONV_SHAPES = [(1, 1, 1, 64, 64, 3, 1, 1), (1, 1, 31, 64, 192, 3, 1, 1), (2, 4, 4, 64, 64, 3, 1, 1), (1, 3, 11, 3, 64, 3, 1, 1),
               (1, 7, 9, 64, 64, 5, 1, 2), (1, 8, 8, 64, 192, 3, 1, 1), (1, 5, 13, 3, 192, 3, 1, 1), (1, 9, 511, 3, 64, 11, 4, 2),
               (2, 8, 8, 64, 64, 3, 1, 1), (1, 3, 43, 64, 64, 5, 1, 2), (1, 257, 1, 64, 64, 3, 1, 1), (2, 31, 35, 3, 64, 11, 4, 2),
               (2, 5, 7, 128, 192, 5, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=["x".join(map(str, s)) for s in CONV_SHAPES])
def test_convolution_alone_against_float64_conv2d(shape):
    N, IH, IW, Cin, Cout, K, stride, pad = shape
    rng = np.random.default_rng(sum(p * v for p, v in zip((1, 3, 5, 7, 11, 13, 17, 19), shape)))
    x = torch.from_numpy(rng.standard_normal((N, Cin, IH, IW)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((Cout, Cin, K, K)) * np.sqrt(2.0 / (Cin * K * K))).astype(np.float32))
    bias = torch.from_numpy((0.1 * rng.standard_normal(Cout)).astype(np.float32))
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=pad))
    dev32 = (F.relu(F.conv2d(x, w, bias, stride=stride, padding=pad)).double() - ref).abs().max().item()
    dev = _device()
    got = D.conv(x.permute(0, 2, 3, 1).contiguous().to(dev), D.pack_conv_weight(w.to(dev)), bias.to(dev), K, stride, pad).permute(0, 3, 1, 2).cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    M = N * ref.shape[2] * ref.shape[3]
    err = (got.double() - ref).abs().max().item()
    print(f"M = {M}: max|fused - f64| = {err:.3e}, float32 conv2d {dev32:.3e}, floor {ULP16(ref.abs().max().item()):.3e}")
    _record("convolution-alone", {"x".join(map(str, shape)): err / max(dev32, ULP16(ref.abs().max().item()))})
    assert err <= gate(dev32, ref.abs().max().item())
    if N == 2:   # image b of a batch is the single call, bit for bit
        for b in range(N):
            one = D.conv(x[b:b + 1].permute(0, 2, 3, 1).contiguous().to(dev), D.pack_conv_weight(w.to(dev)), bias.to(dev), K, stride, pad)
            assert torch.equal(one.permute(0, 3, 1, 2).cpu()[0], got[b])


def test_convolution_shapes_reach_the_pixel_counts_of_the_issue():
    out = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    counts = {N * out(IH, K, s, p) * out(IW, K, s, p) for N, IH, IW, _, _, K, s, p in CONV_SHAPES}
    assert {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257} <= counts
    assert {(s[3], s[4]) for s in CONV_SHAPES} >= {(3, 64), (3, 192), (64, 64), (64, 192)}
    assert {(s[5], s[6], s[7]) for s in CONV_SHAPES} == {(11, 4, 2), (5, 1, 2), (3, 1, 1)} and {s[0] for s in CONV_SHAPES} == {1, 2}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 9, 64, 3), (1, 5, 5, 192, 3), (1, 3, 3, 64, 3), (2, 7, 9, 64, 2), (1, 17, 33, 128, 2), (1, 2, 3, 512, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pool_alone_at_odd_sizes(shape):
    N, IH, IW, Cn, window = shape
    x = torch.from_numpy(np.random.default_rng(IH * IW + Cn).standard_normal((N, Cn, IH, IW)).astype(np.float32))
    ref = F.max_pool2d(x, window, 2)
    got = D.pool(x.permute(0, 2, 3, 1).contiguous().to(_device()), window).permute(0, 3, 1, 2).cpu()
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,Cn", [(1, 1, 1, 64), (2, 3, 5, 192), (1, 17, 16, 384), (3, 16, 17, 256), (1, 2, 2, 512), (1, 33, 31, 128)])
def test_head_alone_and_a_pixel_of_zeros_contributes_exactly_zero(B, h, w, Cn):
    dev = _device()
    rng = np.random.default_rng(B * h * w + Cn)
    f = torch.from_numpy(np.maximum(rng.standard_normal((2 * B, Cn, h, w)), 0).astype(np.float32))
    f[:, :, h // 2, w // 2] = 0                                     # the same pixel of every image: all channels zero
    lin = torch.from_numpy((np.abs(rng.standard_normal((1, Cn, 1, 1))) * 64.0 / Cn).astype(np.float32))
    ref = L.oracle_head(f[:B].double(), f[B:].double(), lin).numpy()
    g0 = f[:B] / (f[:B].pow(2).sum(1, keepdim=True).sqrt() + L.EPS)
    g1 = f[B:] / (f[B:].pow(2).sum(1, keepdim=True).sqrt() + L.EPS)
    dev32 = np.abs((((g0 - g1) ** 2) * lin).sum(1).mean((1, 2)).double().numpy() - ref)
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    got = D.head(cl(f), lin.reshape(-1).to(dev)).cpu().numpy()
    assert got.shape == (B,) and np.isfinite(got).all()
    _record("head-alone", {f"{B}x{h}x{w}x{Cn}": max(abs(float(got[b]) - ref[b]) / max(float(dev32[b]), ULP16(ref[b])) for b in range(B))})
    for b in range(B):
        assert abs(float(got[b]) - ref[b]) <= gate(dev32[b], ref[b]), (b, got[b], ref[b])
    # only the zero pixel differs from ... nothing: identical images, a zero pixel among them, give exactly 0 and no NaN
    same = torch.cat((f[:B], f[:B]))
    assert bool((D.head(cl(same), lin.reshape(-1).to(dev)) == 0).all())
    assert bool((D.head(cl(torch.zeros_like(f)), lin.reshape(-1).to(dev)) == 0).all())
    # the zero pixel adds nothing: with every OTHER pixel's features equal in both images, the value is exactly 0 whatever the weights
    lone = same.clone()
    lone[B:, :, h // 2, w // 2] = 0
    assert bool((D.head(cl(lone), 1000 * lin.reshape(-1).to(dev)) == 0).all())


@pytest.mark.gpu
def test_the_opt_in_serves_compute_metrics_of_an_evaluation_module_with_a_filled_cache():
    import wg_integration
    m = L.stand_in_evaluation_module(nets=("alex", "vgg"))
    ca, aa = GOLDEN[IDS.index("alex-35x67")]
    pred, gt = L.make_images(ca)
    to_hwc = lambda t: np.ascontiguousarray(t[0].permute(1, 2, 0).numpy())
    p, g = to_hwc(pred), to_hwc(gt)
    plain = m.compute_metrics(p, g, run_lpips_vgg=True)
    n = len(m.original_calls)
    assert n == 2 and m.built == []
    undo = wg_integration.fuse_evaluation_lpips(m)
    try:
        fused = m.compute_metrics(p, g, run_lpips_vgg=True)
        assert len(m.original_calls) == n and m.built == []            # neither call reached the original; nothing was constructed
        assert set(fused) == set(plain) and fused["mse"] == plain["mse"] and type(fused["lpips"]) is float
        # compute_metrics hands (gt, pred): the oracle's value with the arguments in that order is the same
        ref = L.oracle(L.make_weights("alex"), "alex", gt, pred)[0].numpy()[0]
        assert abs(ref - aa["total64"][0]) <= 1e-12
        assert abs(fused["lpips"] - ref) <= gate(aa["total32_dev"][0], ref)
        assert abs(fused["lpips"] - plain["lpips"]) <= 2 * gate(aa["total32_dev"][0], ref)
        ref_vgg = L.oracle(L.make_weights("vgg"), "vgg", gt, pred)[0].numpy()[0]
        assert abs(fused["lpips_vgg"] - ref_vgg) <= gate(0.0, ref_vgg)
        per_image = m.compute_metrics(np.stack([p, g]), np.stack([g, g]), reduce=False)["lpips"]
        assert per_image.dtype == np.float32 and per_image.shape == (2,) and per_image[1] == 0 and abs(per_image[0] - ref) <= gate(aa["total32_dev"][0], ref)
        small = np.zeros((20, 40, 3), np.float32)
        with pytest.raises(RuntimeError):
            m.lpips(small, small)                                      # under alex's minimum: the caller's own function, whose pool refuses it
        assert len(m.original_calls) == n + 1 and m.original_calls[-1][0] is small
    finally:
        undo()
    m.compute_metrics(p, g)
    assert len(m.original_calls) == n + 2                              # undone: the original again
