"""The fused toned-colour operator (include/wg_appearance_colour.h, wg_fused_gaussians.toned_colours / fit_appearance_embedding) against the
float64 oracle of tests/appearance_colour_lib.py.  The gate everywhere is |kernel - float64| <= the oracle's a-priori float32 rounding
bound, element by element: no tuned tolerance, no excluded elements.

GPU shapes are the smallest at which the tile walk can go wrong: a tile is 64 list entries walked as two halves of 32, so M = 1, 63, 64, 65
and 5 tiles + 37 with max_workgroups = 3 give idle workgroups, a ragged half, a ragged tile, workgroups with two tiles and one with a ragged
last tile; widths 6 / 5 are no multiple of the MFMA's K; the row list is scattered and unsorted over twice as many rows."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import appearance_colour_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wg_appearance_colour.h")
INF = float("inf")


def FG():
    import wg_fused_gaussians
    return wg_fused_gaussians


@functools.lru_cache(maxsize=None)
def case(P, G, E, seed, pre=1.0, post=1.0):
    return L.make_case(P, G, E, seed, pre, post)


# ---- CPU: the C-ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_names_are_exported_and_nothing_else():
    names = set(re.findall(r"\b(wg_appearance_colour_\w+)\s*\(", open(HEADER).read()))
    assert names == {"wg_appearance_colour_scratch_floats", "wg_appearance_colour_forward", "wg_appearance_colour_backward"}
    lib = FG()._lib._name
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("wg_appearance_colour")}
    assert exported == names


def test_scratch_size_arithmetic():
    fg = FG()
    f = fg._lib.wg_appearance_colour_scratch_floats
    macros = dict(re.findall(r"#define (WG_COLOUR_\w+) +(\d+)\b", open(HEADER).read()))
    assert int(macros["WG_COLOUR_TILE_ROWS"]) == fg.COLOUR_TILE_ROWS == 64 and int(macros["WG_COLOUR_PARTIAL_FLOATS"]) == fg.COLOUR_PARTIAL_FLOATS == 128
    assert int(macros["WG_COLOUR_COEFFS"]) == fg.COLOUR_COEFFS == 48
    for M in (0, 1, 63, 64, 65, 128, 129, 1000, 3_000_000):
        for wgs in (1, 3, 7, 256):
            assert f(M, wgs) == min((M + 63) // 64, wgs) * 128, (M, wgs)
    assert f(0, 0) == 0   # no tile: no device is asked
    assert f(-1, 3) < 0 and f(10, -1) < 0
    assert C.sizeof(fg._ColourArgs) == 28 * 8   # the header's struct, field by field, on an LP64 host


def _valid_args(fg, P=400, M=200, G=24, E=32, wgs=3, rows=True):
    """A well-formed argument block over FAKE device addresses: every call made with it must be refused before any device work."""
    a = fg._ColourArgs()
    fake = 0x10000
    a.struct_size = C.sizeof(fg._ColourArgs)
    a.P, a.M, a.rows = P, M, (fake if rows else None)
    a.features, a.features_row_stride, a.deg = fake, 48, 3
    a.gembedding_width, a.gembedding, a.gembedding_row_stride = G, fake, G + 2
    a.shared, a.shared_width, a.max_workgroups = fake, E, wgs
    a.xyz, a.xyz_row_stride, a.campos = fake, 3, fake
    a.W1 = a.b1 = a.W2 = a.b2 = a.W3 = a.b3 = fake
    a.out_scale, a.pre_clamp_max, a.post_clamp_max = 0.01, 1.0, 1.0
    a.colours = a.dL_dcolours = a.grad_shared = a.scratch = fake
    a.scratch_floats = fg._lib.wg_appearance_colour_scratch_floats(M, wgs)
    return a


def _no_rows_more_than_P(a):
    a.rows, a.M = None, a.P + 1
    a.scratch_floats = 10 ** 9


MALFORMED = {
    "struct_size short": lambda a: setattr(a, "struct_size", a.struct_size - 8),
    "P negative": lambda a: setattr(a, "P", -1),
    "M negative": lambda a: setattr(a, "M", -1),
    "M > P without rows": _no_rows_more_than_P,
    "null features": lambda a: setattr(a, "features", None),
    "features stride 47": lambda a: setattr(a, "features_row_stride", 47),
    "deg 4": lambda a: setattr(a, "deg", 4),
    "deg negative": lambda a: setattr(a, "deg", -1),
    "G 62": lambda a: (setattr(a, "gembedding_width", 62), setattr(a, "gembedding_row_stride", 62)),
    "G negative": lambda a: setattr(a, "gembedding_width", -1),
    "null gembedding": lambda a: setattr(a, "gembedding", None),
    "gembedding stride < G": lambda a: setattr(a, "gembedding_row_stride", 23),
    "null shared": lambda a: setattr(a, "shared", None),
    "E 0": lambda a: setattr(a, "shared_width", 0),
    "E 65": lambda a: setattr(a, "shared_width", 65),
    "null xyz": lambda a: setattr(a, "xyz", None),
    "xyz stride 2": lambda a: setattr(a, "xyz_row_stride", 2),
    "null campos": lambda a: setattr(a, "campos", None),
    "null W1": lambda a: setattr(a, "W1", None),
    "null b2": lambda a: setattr(a, "b2", None),
    "null b3": lambda a: setattr(a, "b3", None),
    "max_workgroups negative": lambda a: setattr(a, "max_workgroups", -2),
}
MALFORMED_FWD = {"null colours": lambda a: setattr(a, "colours", None)}
MALFORMED_BWD = {
    "null dL_dcolours": lambda a: setattr(a, "dL_dcolours", None),
    "null grad_shared": lambda a: setattr(a, "grad_shared", None),
    "null scratch": lambda a: setattr(a, "scratch", None),
    "scratch one float short": lambda a: setattr(a, "scratch_floats", a.scratch_floats - 1),
    "scratch sized for fewer workgroups": lambda a: setattr(a, "max_workgroups", 4),   # M = 200: 4 tiles, sized for 3 workgroups
}


@pytest.mark.parametrize("which", sorted(MALFORMED) + sorted(MALFORMED_FWD))
def test_malformed_forward_refused_before_device_work(which):
    fg = FG()
    a = _valid_args(fg)
    {**MALFORMED, **MALFORMED_FWD}[which](a)
    assert fg._lib.wg_appearance_colour_forward(C.byref(a)) == -1   # WG_ERR_INVALID_ARGUMENT; a launch on these addresses would be WG_ERR_HIP or a fault


@pytest.mark.parametrize("which", sorted(MALFORMED) + sorted(MALFORMED_BWD))
def test_malformed_backward_refused_before_device_work(which):
    fg = FG()
    a = _valid_args(fg)
    {**MALFORMED, **MALFORMED_BWD}[which](a)
    assert fg._lib.wg_appearance_colour_backward(C.byref(a)) == -1


def test_null_argument_block_refused():
    fg = FG()
    assert fg._lib.wg_appearance_colour_forward(None) == -1 and fg._lib.wg_appearance_colour_backward(None) == -1


# ---- CPU: the Python entry -----------------------------------------------------------------------------------------------------------------
def _cpu_inputs(P=4, G=24, E=32, dtype=torch.float32):
    W = [w.to(dtype) for w in L.draw_weights(3 + G + E, 1)]
    return dict(features=torch.zeros(P, 48, dtype=dtype), gembedding=torch.zeros(P, G, dtype=dtype), embedding=torch.zeros(E, dtype=dtype),
                xyz=torch.ones(P, 3, dtype=dtype), campos=torch.zeros(3, dtype=dtype), weights=W, deg=3)


@pytest.mark.parametrize("which", ["features", "gembedding", "xyz", "campos", "weights"])
def test_an_input_that_requires_a_gradient_is_refused(which):
    kw = _cpu_inputs()
    if which == "weights":
        kw["weights"][2].requires_grad_(True)
    else:
        kw[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="detach"):
        FG().toned_colours(**kw)


def test_cpu_tensors_and_other_dtypes_are_refused():
    with pytest.raises(RuntimeError, match="no CPU path"):
        FG().toned_colours(**_cpu_inputs())
    with pytest.raises(RuntimeError, match="float32"):
        FG().toned_colours(**_cpu_inputs(dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        FG().toned_colours(**dict(_cpu_inputs(), deg=4))


# ---- CPU: the oracle ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 357)
WIDTHS = ((24, 32), (6, 5))
# (M, G, E, seed, listed): listed = False is rows = None over P = M rows; True a scattered list of M among P = 2 M rows
ALL_CASES = [(M, G, E, 300 + 10 * i + j, listed) for i, (G, E) in enumerate(WIDTHS) for j, M in enumerate(SIZES) for listed in (False, True)]
EXTRA_CASES = [(357, 24, 32, 401, 1.0, INF), (357, 24, 32, 402, INF, INF), (357, 24, 32, 403, 1.25, 0.75), (714, 24, 32, 404, 1.0, 1.0)]


def _P(M, listed):
    return 2 * M if listed else M


def test_robust_row_cap_and_every_branch_exercised():
    cases = [case(_P(M, listed), G, E, seed) for M, G, E, seed, listed in ALL_CASES]
    cases += [case(P, G, E, seed) for P, G, E, seed, _ in L.GOLDEN_CASES] + [case(*a) for a in EXTRA_CASES]
    for c in cases:
        assert c["discarded"] < L.MAX_DISCARD, (c["P"], c["G"], c["E"], c["seed"], c["discarded"], c["lost"])
        ok, _ = L.robust(c["features"], c["gemb"], c["emb"], c["xyz"], c["campos"], [w.double() for w in c["weights"]], c["pre"], c["post"])
        assert bool(ok.all())
    c = case(357, 24, 32, ALL_CASES[8][3])
    o = L.oracle(c, L.dense_cotangent(357, 1), 3)
    assert 0.05 < o["clamped"] < 0.6 and 0.03 < o["floored"] < 0.5, (o["clamped"], o["floored"])
    assert float((o["om"][:, 3:] - 1).abs().mean()) < 0.5   # mul near 1


def _golden():
    z = np.load(L.GOLDEN)
    assert [tuple(x) for x in json.loads(str(z["cases"]))] == [tuple(x) for x in L.GOLDEN_CASES]
    return z


@pytest.mark.parametrize("i", range(len(L.GOLDEN_CASES)))
def test_oracle_is_pinned_to_the_reference_fixture(i):
    z = _golden()
    P, G, E, seed, deg = L.GOLDEN_CASES[i]
    o = L.oracle(case(P, G, E, seed), L.golden_cot(P, seed), deg, scale=0.01)   # the fixture's float64 arrays were computed with the double constant
    for k in ("colours", "grad"):
        want64 = torch.from_numpy(z[f"{k}64_{i}"])
        assert want64.dtype == torch.float64 and want64.shape == o[k].shape
        assert float(((o[k] - want64).abs() / want64.abs().clamp_min(1.0)).max()) <= 1e-12, k   # the oracle restates the reference
        got32 = torch.from_numpy(z[f"{k}32_{i}"])
        assert got32.dtype == torch.float32
        assert L.ratio(got32, o[k], o["e_" + k]) <= 1.0, k                                       # and PyTorch's float32 is within the bound


def test_oracle_against_the_reference_statements():
    checkout = os.environ.get("WG_REFERENCE_CHECKOUT", "/root/reference")
    if not os.path.exists(os.path.join(checkout, "wildgaussians", "method.py")):
        pytest.skip("no checkout of the reference on this machine")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_appearance_colour_golden", os.path.join(ROOT, "tests", "golden", "make_appearance_colour_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    cls, eval_sh = mk.reference_parts(checkout)
    c = case(65, 24, 32, 999)
    for deg in range(4):
        o = L.oracle(c, L.golden_cot(65, 999), deg, scale=0.01)
        for dtype in (torch.float64, torch.float32):
            colours, grad = L.run_reference(mk.reference_model(cls, c, dtype), eval_sh, c, deg, dtype)
            for k, got in (("colours", torch.from_numpy(colours)), ("grad", torch.from_numpy(grad))):
                if dtype == torch.float64:
                    assert float(((o[k] - got).abs() / got.abs().clamp_min(1.0)).max()) <= 1e-12, (deg, k)
                else:
                    assert L.ratio(got, o[k], o["e_" + k]) <= 1.0, (deg, k)


def test_plain_pytorch_chain_restates_the_oracle():
    """appearance_colour_lib.torch_chain (the bench's and the accuracy record's PyTorch leg) in float64 is the oracle's value."""
    c = case(65, 24, 32, 999)
    W = [w.double() for w in c["weights"]]
    for deg in range(4):
        o = L.oracle(c, L.golden_cot(65, 999), deg, scale=0.01)
        got = L.torch_chain(c["features"].double(), c["gemb"].double(), c["emb"].double(), c["xyz"].double(), c["campos"].double(), W, deg)
        assert float((got - o["colours"]).abs().max()) <= 1e-12


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _device_inputs(c, features=None):
    dev = "cuda"
    return dict(features=c["features"].to(dev) if features is None else features, gembedding=c["gemb"].to(dev), xyz=c["xyz"].to(dev),
                campos=c["campos"].to(dev), weights=[w.to(dev) for w in c["weights"]])


def _run(c, cot, deg, rows=None, max_workgroups=3, features=None):
    """toned_colours forward + backward on the device -> (colours [P, 3], grad [E])."""
    emb = c["emb"].to("cuda").requires_grad_(True)
    out = FG().toned_colours(embedding=emb, deg=deg, rows=None if rows is None else rows.to("cuda"), pre_clamp_max=c["pre"],
                             post_clamp_max=c["post"], max_workgroups=max_workgroups, **_device_inputs(c, features))
    assert out.shape == (c["P"], 3) and out.dtype == torch.float32
    out.backward(cot.to("cuda"))
    return out.detach(), emb.grad


def _assert_within(got, o, tag=""):
    for k, v in zip(("colours", "grad"), got):
        q = L.ratio(v, o[k], o["e_" + k])
        print(f"{tag} {k}: max err/bound {q:.4f}")
        assert q <= 1.0, (tag, k, q)


def _check(M, G, E, seed, listed, deg, cot_of=L.dense_cotangent, max_workgroups=3, pre=1.0, post=1.0):
    P = _P(M, listed)
    c = case(P, G, E, seed, pre, post)
    rows = L.scattered_rows(P, M, seed) if listed else None
    cot = cot_of(P, seed)
    o = L.oracle(c, cot, deg, rows)
    got = _run(c, cot, deg, rows, max_workgroups)
    _assert_within(got, o, tag=f"M={M} P={P} G={G} E={E} deg={deg} listed={listed}")
    if listed:   # rows not listed are exact zeros
        off = torch.ones(P, dtype=torch.bool)
        off[rows] = False
        assert bool((got[0].cpu()[off] == 0).all())
    return c, rows, cot, o, got


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("M,G,E,seed,listed", ALL_CASES, ids=[f"M{c[0]}-G{c[1]}-E{c[2]}-{'list' if c[4] else 'all'}" for c in ALL_CASES])
def test_forward_backward_within_bound(M, G, E, seed, listed, deg):
    _check(M, G, E, seed, listed, deg)


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("M,G,E,seed,listed", ALL_CASES[6:8] + ALL_CASES[16:18], ids=["G24-all", "G24-list", "G6-all", "G6-list"])
def test_degrees_one_and_two(M, G, E, seed, listed, deg):
    assert M == 65
    _check(M, G, E, seed, listed, deg)


@pytest.mark.gpu
def test_automatic_grid():
    fg = FG()
    wgs = fg.appearance_colour_scratch_floats(10 ** 9, 0) // fg.COLOUR_PARTIAL_FLOATS
    assert wgs >= 1
    M = 64 * wgs + 37   # every workgroup a tile, the first a second, ragged one
    for listed in (False, True):
        _check(M, 24, 32, 4242, listed, 3, max_workgroups=0)
        _check(M, 24, 32, 4242, listed, 3, cot_of=L.sparse_cotangent, max_workgroups=0)


@pytest.mark.gpu
@pytest.mark.parametrize("listed", [False, True], ids=["all", "list"])
def test_sparse_cotangent_shows_a_lost_tile(listed):
    """One row per 64 plus the first and the last: n is 8, and the yardstick sees one lost row."""
    M, G, E, seed = 357, 24, 32, ALL_CASES[8][3] if not listed else ALL_CASES[9][3]
    c, rows, cot, o, _ = _check(M, G, E, seed, listed, 3, cot_of=L.sparse_cotangent)
    idx = torch.arange(c["P"]) if rows is None else rows
    live = [int(r) for r in idx if bool((cot[r] != 0).any()) and bool((o["colours"][r] > 0).any())]
    cot2 = cot.clone()
    cot2[live[len(live) // 2]] = 0
    o2 = L.oracle(c, cot2, 3, rows)
    lost = L.ratio(o2["grad"], o["grad"], o["e_grad"])
    print(f"a lost row under the sparse cotangent: {lost:.1f} x the bound")
    assert lost > 10.0


@pytest.mark.gpu
def test_strided_features_view_is_read_in_place():
    M, G, E, seed, listed = ALL_CASES[9]
    P = _P(M, listed)
    c = case(P, G, E, seed)
    rows, cot = L.scattered_rows(P, M, seed), L.dense_cotangent(P, seed)
    wide = torch.full((P, 80), float("nan"), device="cuda")
    wide[:, 7:55] = c["features"].to("cuda")
    view = wide[:, 7:55]
    assert not view.is_contiguous() and FG()._colour_row_view(view, 48, "features").data_ptr() == view.data_ptr()
    _assert_within(_run(c, cot, 3, rows, features=view), L.oracle(c, cot, 3, rows), tag="strided")


@pytest.mark.gpu
@pytest.mark.parametrize("P,G,E,seed,pre,post", EXTRA_CASES[:3], ids=["post-inf", "both-inf", "pre1.25-post0.75"])
def test_other_clamp_bounds(P, G, E, seed, pre, post):
    c = case(P, G, E, seed, pre, post)
    cot = L.dense_cotangent(P, seed)
    o = L.oracle(c, cot, 3)
    assert (o["clamped"] == 0) == (post == INF)
    _assert_within(_run(c, cot, 3), o, tag=f"pre={pre} post={post}")


@pytest.mark.gpu
@pytest.mark.parametrize("max_workgroups", [3, 0])
def test_two_calls_give_the_same_bits(max_workgroups):
    M, G, E, seed, listed = ALL_CASES[9]
    P = _P(M, listed)
    c = case(P, G, E, seed)
    rows, cot = L.scattered_rows(P, M, seed), L.dense_cotangent(P, seed)
    a, b = _run(c, cot, 3, rows, max_workgroups), _run(c, cot, 3, rows, max_workgroups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _raw_args(fg, c, rows, deg, keep):
    t = _device_inputs(c)
    emb = c["emb"].to("cuda")
    idx = rows.to("cuda", torch.int32)
    a = fg._ColourArgs()
    fg._colour_fill(a, t["features"], t["gembedding"], emb, t["xyz"], t["campos"], idx, idx.numel(), t["weights"], deg, 1.0, 1.0, 0.01, 3,
                    torch.cuda.current_stream().cuda_stream)
    keep += [t, emb, idx]
    return a


@pytest.mark.gpu
def test_unlisted_rows_are_neither_written_nor_read():
    fg = FG()
    M, G, E, seed, listed = ALL_CASES[9]
    P = _P(M, listed)
    c = case(P, G, E, seed)
    rows, cot = L.scattered_rows(P, M, seed), L.dense_cotangent(P, seed)
    o = L.oracle(c, cot, 3, rows)
    off = torch.ones(P, dtype=torch.bool)
    off[rows] = False
    keep = []
    a = _raw_args(fg, c, rows, 3, keep)
    sentinel = -12345.0
    colours = torch.full((P, 3), sentinel, device="cuda")
    a.colours = colours.data_ptr()
    assert fg._lib.wg_appearance_colour_forward(C.byref(a)) == 0
    torch.cuda.synchronize()
    assert bool((colours.cpu()[off] == sentinel).all())
    assert L.ratio(colours.cpu()[rows], o["colours"][rows], o["e_colours"][rows]) <= 1.0
    # backward: whatever the cotangent of an unlisted row holds, no bit of the gradient changes
    g1 = _run(c, cot, 3, rows)[1]
    loud = cot.clone()
    loud[off] = 1e30
    loud[off.nonzero()[0]] = float("nan")
    g2 = _run(c, loud, 3, rows)[1]
    assert torch.equal(g1, g2)
    assert L.ratio(g2, o["grad"], o["e_grad"]) <= 1.0


@pytest.mark.gpu
def test_fused_and_unfused_chain_agree_through_one_oracle():
    fg = FG()
    P, G, E, seed = 357, 24, 32, ALL_CASES[8][3]
    c = case(P, G, E, seed)
    cot = L.dense_cotangent(P, seed)
    o = L.oracle(c, cot, 3)
    _assert_within(_run(c, cot, 3, torch.arange(P)), o, tag="fused, rows = all")
    t = _device_inputs(c)
    emb = c["emb"].to("cuda").requires_grad_(True)
    out = L.operator_chain(fg, t["features"], t["gembedding"], emb, t["xyz"], t["campos"], t["weights"], 3, max_workgroups=3)
    out.backward(cot.to("cuda"))
    _assert_within((out.detach(), emb.grad), o, tag="appearance_mlp + tone + eval_sh")


@pytest.mark.gpu
def test_empty_list():
    c = case(65, 24, 32, ALL_CASES[6][3])
    got = _run(c, L.dense_cotangent(65, 1), 3, torch.zeros(0, dtype=torch.int64))
    assert bool((got[0] == 0).all()) and bool((got[1] == 0).all()) and got[1].shape == (32,)


@pytest.mark.gpu
def test_mask_and_row_list_are_reusable():
    fg = FG()
    M, G, E, seed, listed = ALL_CASES[7]
    P = _P(M, listed)
    c = case(P, G, E, seed)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[L.scattered_rows(P, M, seed)] = True
    rl = fg.RowList(mask.cuda())
    assert rl.M == M and rl.index.dtype == torch.int32
    cot = L.dense_cotangent(P, seed)
    o = L.oracle(c, cot, 3, mask.nonzero()[:, 0])
    emb = c["emb"].cuda().requires_grad_(True)
    for rows in (mask.cuda(), rl, rl):
        emb.grad = None
        out = fg.toned_colours(embedding=emb, deg=3, rows=rows, max_workgroups=3, **_device_inputs(c))
        out.backward(cot.cuda())
        _assert_within((out.detach(), emb.grad), o, tag="mask / RowList")


# ---- GPU: fit_appearance_embedding ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_scene():
    """300 Gaussians in a 64 x 64 image; the ground truth is the render under another embedding.  Large splats and a tone whose offset and mul
    both move with the embedding, so that most of the E elements carry a gradient well above 1e-5."""
    import wg_scenes as S
    from diff_gaussian_rasterization import GaussianRasterizer
    from wg_testlib import make_settings, to_dev
    P, Wd, H, G, E = 300, 64, 64, 24, 32
    cam = S.make_camera(Wd, H)
    cloud = S.make_cloud(P, Wd, H, sh_degree=None, seed=5, scale_mult=12.0)
    rast = GaussianRasterizer(make_settings(cam, 3))
    g = torch.Generator().manual_seed(9)
    t = dict(means3D=to_dev(cloud["means3D"]), opacities=to_dev(cloud["opacities"]), scales=to_dev(cloud["scales"]), rotations=to_dev(cloud["rotations"]),
             features=(torch.rand(P, 48, generator=g) * 1.75 - 0.25).cuda(), gembedding=(torch.rand(P, G, generator=g) * 2 - 1).cuda())
    W = L.draw_weights(3 + G + E, 17)
    W[0][:, 3 + G:] *= 6       # the embedding's columns: the image depends on it strongly
    W[4] = W[4] * 40
    weights = [w.cuda() for w in W]
    emb0, emb_gt = (torch.randn(E, generator=g) * 0.3).cuda(), (torch.randn(E, generator=g) * 0.3).cuda()
    with torch.no_grad():
        col = FG().toned_colours(t["features"], t["gembedding"], emb_gt, t["means3D"], rast.raster_settings.campos, weights, 3)
        gt = rast(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], colors_precomp=col, scales=t["scales"],
                  rotations=t["rotations"])[0]
    return rast, t, weights, emb0, gt


def _unfused_gradient(rast, t, weights, emb0, gt, loss):
    from wg_fused_ssim import l1_ssim_loss
    emb = emb0.clone().requires_grad_(True)
    col = L.operator_chain(FG(), t["features"], t["gembedding"], emb, t["means3D"], rast.raster_settings.campos, weights, 3)
    image = rast(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], colors_precomp=col, scales=t["scales"],
                 rotations=t["rotations"])[0]
    value = torch.nn.functional.mse_loss(image, gt) if loss == "mse" else l1_ssim_loss(image, image, gt, 0.2)
    value.backward()
    return emb.grad


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["dssim+l1", "mse"])
def test_fit_first_step_follows_the_unfused_gradient(loss):
    rast, t, weights, emb0, gt = _fit_scene()
    lr = 0.1
    g_ref = _unfused_gradient(rast, t, weights, emb0, gt, loss)
    emb, losses, mses = FG().fit_appearance_embedding(rast, t["means3D"], t["opacities"], t["scales"], t["rotations"], t["features"], t["gembedding"],
                                                      weights, emb0, gt, iters=1, lr=lr, loss=loss)
    assert losses.shape == (1,) and mses.shape == (1,) and not losses.is_cuda
    ok = g_ref.abs() >= 1e-5
    print(f"{loss}: {int(ok.sum())} of {ok.numel()} elements qualify; |g_ref| median {float(g_ref.abs().median()):.2e}")
    assert int(ok.sum()) * 2 >= ok.numel()
    dev = ((emb - emb0) + lr * torch.sign(g_ref)).abs()[ok]
    print(f"largest deviation from -lr sign(g_ref): {float(dev.max()):.3e}")
    assert float(dev.max()) <= 2e-3 * lr


@pytest.mark.gpu
def test_fit_descends_and_scales_the_cotangent():
    rast, t, weights, emb0, gt = _fit_scene()
    args = (rast, t["means3D"], t["opacities"], t["scales"], t["rotations"], t["features"], t["gembedding"], weights, emb0, gt)
    emb, losses, mses = FG().fit_appearance_embedding(*args, iters=16, lr=0.02)
    print("losses", [round(float(x), 5) for x in losses])
    assert losses.shape == (16,) and float(losses[-1]) < float(losses[0]) and float(mses[-1]) < float(mses[0])
    # grad_scale: the image's value (so the first loss) unchanged; a zero scale leaves the embedding where it was
    emb_z, losses_z, _ = FG().fit_appearance_embedding(*args, iters=1, lr=0.02, grad_scale=torch.zeros(1, 64, 64, device="cuda"))
    # (the same float32 sums, possibly in another order between two runs: a few units of 2^-24, far inside 1e-6)
    assert abs(float(losses_z[0]) - float(losses[0])) <= 1e-6 * float(losses[0]) and torch.equal(emb_z, emb0)
