"""The appearance MLP over a list of rows and the device-side compaction that builds the list (include/wg_appearance_rows.h,
wg_fused_gaussians.VisibleRows / appearance_mlp(rows=) / embedding_forward(rows=) / appearance_rows).

The central gate has no tolerance: entry i of the list takes the place of row i in the dense walk, so every output must have the BITS of
the dense operator (tests/test_appearance_mlp.py holds that one to the float64 oracle) run on gathered copies of the inputs.  Shapes are
the smallest at which the walk can go wrong: lists around the 32-entry half tile and the 64-entry tile, several tiles per workgroup with a
ragged end (max_workgroups 2 and 3), an empty list, a shuffled list; compaction sizes around the wave (64), the workgroup pass (256) and
the 2048-entry block (P = 5000: three blocks)."""
import ctypes as C
import functools
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import appearance_mlp_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wg_appearance_rows.h")
WNAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]
CASE = (357, 24, 32, 104)
OFF = dict(ssim=False, adam=False, densification_stats=False, activations=False, eval_sh=False, geometry_reuse=False)


def FG():
    import wg_fused_gaussians
    return wg_fused_gaussians


@functools.lru_cache(maxsize=None)
def case(P, G, E, seed):
    return L.make_case(P, G, E, seed)


# ---- CPU: the C-ABI ----------------------------------------------------------------------------------------------------------------------
NAMES = {"wg_appearance_rows_scratch_floats", "wg_appearance_rows_forward", "wg_appearance_rows_backward",
         "wg_appearance_rows_compact_scratch_bytes", "wg_appearance_rows_compact"}


def test_header_names_are_exported_and_nothing_else():
    names = set(re.findall(r"\b(wg_appearance_rows_\w+)\s*\(", open(HEADER).read()))
    assert names == NAMES
    out = subprocess.run(["nm", "-D", "--defined-only", FG()._lib._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("wg_appearance_rows")}
    assert exported == names


def test_scratch_size_arithmetic():
    fg = FG()
    f, g = fg._lib.wg_appearance_rows_scratch_floats, fg._lib.wg_appearance_rows_compact_scratch_bytes
    macros = dict(re.findall(r"#define (WG_ROWS_\w+) +(\d+)\b", open(HEADER).read()))
    assert int(macros["WG_ROWS_COMPACT_BLOCK"]) == fg.ROWS_COMPACT_BLOCK == 2048
    for M in (0, 1, 63, 64, 65, 128, 129, 1000, 3_000_000, 2 ** 31 - 1):
        for wgs in (1, 3, 7, 256):
            assert f(M, wgs) == fg.MLP_SCRATCH_HEAD_FLOATS + min((M + 63) // 64, wgs) * fg.MLP_PARTIAL_FLOATS, (M, wgs)
            assert M > 3_000_000 or f(M, wgs) == fg._lib.wg_appearance_mlp_scratch_floats(M, wgs)
    assert f(0, 0) == fg.MLP_SCRATCH_HEAD_FLOATS   # no tile: no device is asked
    assert f(-1, 3) < 0 and f(10, -1) < 0 and f(2 ** 31, 3) < 0
    for P in (0, 1, 2047, 2048, 2049, 5000, 3_000_000, 2 ** 31 - 1):
        assert g(P) == 4 * max(1, (P + 2047) // 2048), P
    assert g(-1) < 0 and g(2 ** 31) < 0


def _valid_args(fg, P=300, M=200, wgs=3, count=False, **kw):
    """A well-formed argument block over FAKE device addresses: every call made with it must be refused before any device work."""
    import test_appearance_mlp as T
    m = T._valid_args(fg, P=P, wgs=wgs, **kw)
    a = fg._RowsArgs()
    C.memmove(C.byref(a.mlp), C.byref(m), C.sizeof(m))
    a.struct_size = C.sizeof(fg._RowsArgs)
    a.rows, a.M, a.rows_count = 0x10000, M, (0x10000 if count else None)
    a.mlp.scratch_floats = fg._lib.wg_appearance_rows_scratch_floats(M, wgs)
    return a


def _malformed():
    import test_appearance_mlp as T
    on_mlp = lambda fn: (lambda a: fn(a.mlp))   # noqa: E731
    both = {"mlp: " + k: on_mlp(v) for k, v in T.MALFORMED.items()}
    both.update({
        "struct_size short": lambda a: setattr(a, "struct_size", a.struct_size - 8),
        "null rows": lambda a: setattr(a, "rows", None),
        "M negative": lambda a: setattr(a, "M", -1),
        "M 2^31": lambda a: setattr(a, "M", 2 ** 31),
    })
    fwd = {"mlp: " + k: on_mlp(v) for k, v in T.MALFORMED_FWD.items()}
    bwd = {"mlp: " + k: on_mlp(v) for k, v in T.MALFORMED_BWD.items()}
    # 200 entries are 4 tiles on 3 workgroups; 128 entries are 2 tiles on 2
    bwd["scratch sized for a shorter list"] = lambda a: setattr(a.mlp, "scratch_floats", FG()._lib.wg_appearance_rows_scratch_floats(128, 3))
    return both, fwd, bwd


_BOTH_KEYS = ["mlp: " + k for k in ("struct_size short", "P negative", "no segments", "four segments", "null segment", "width 0", "widths sum 65",
                                     "row_stride < width", "shared_width 65", "shared_width negative", "shared null with a width", "null W1",
                                     "null b2", "null W3", "max_workgroups negative")] + ["struct_size short", "null rows", "M negative", "M 2^31"]
_FWD_KEYS = ["mlp: null out"]
_BWD_KEYS = ["mlp: " + k for k in ("null dL_dout", "five weight gradients", "one weight gradient", "grad stride < width", "null scratch",
                                    "scratch one float short", "scratch sized for fewer workgroups")] + ["scratch sized for a shorter list"]


def test_malformed_tables_cover_the_dense_operator_s():
    both, fwd, bwd = _malformed()
    assert sorted(both) == sorted(_BOTH_KEYS) and sorted(fwd) == sorted(_FWD_KEYS) and sorted(bwd) == sorted(_BWD_KEYS)


@pytest.mark.parametrize("count", [False, True], ids=["host-count", "device-count"])
@pytest.mark.parametrize("which", _BOTH_KEYS + _FWD_KEYS)
def test_malformed_forward_refused_before_device_work(which, count):
    fg = FG()
    both, fwd, _ = _malformed()
    a = _valid_args(fg, count=count)
    {**both, **fwd}[which](a)
    assert fg._lib.wg_appearance_rows_forward(C.byref(a)) == -1   # WG_ERR_INVALID_ARGUMENT; a launch on these addresses would be WG_ERR_HIP or a fault


@pytest.mark.parametrize("count", [False, True], ids=["host-count", "device-count"])
@pytest.mark.parametrize("which", _BOTH_KEYS + _BWD_KEYS)
def test_malformed_backward_refused_before_device_work(which, count):
    fg = FG()
    both, _, bwd = _malformed()
    a = _valid_args(fg, count=count)
    {**both, **bwd}[which](a)
    assert fg._lib.wg_appearance_rows_backward(C.byref(a)) == -1


def test_null_argument_block_refused():
    fg = FG()
    assert fg._lib.wg_appearance_rows_forward(None) == -1 and fg._lib.wg_appearance_rows_backward(None) == -1


def test_malformed_compaction_refused_before_device_work():
    f = FG()._lib.wg_appearance_rows_compact
    k = 0x10000
    assert f(-1, k, None, k, k, k, 4096, None) == -1              # P < 0
    assert f(2 ** 31, k, None, k, k, k, 1 << 40, None) == -1      # P > 2^31 - 1
    assert f(5000, k, k, k, k, k, 4096, None) == -1               # both inputs
    assert f(5000, None, None, k, k, k, 4096, None) == -1         # neither
    assert f(5000, k, None, None, k, k, 4096, None) == -1         # null rows
    assert f(5000, None, k, k, None, k, 4096, None) == -1         # null count
    assert f(5000, None, k, k, k, None, 4096, None) == -1         # null scratch
    assert f(5000, k, None, k, k, k, 8, None) == -1               # three blocks need 12 bytes
    assert f(0, None, None, None, None, k, 4, None) == -1         # P = 0 still writes the count


# ---- CPU: the context manager --------------------------------------------------------------------------------------------------------------
def test_context_manager_nests_restores_and_is_empty_by_default():
    fg = FG()
    assert fg.current_appearance_rows() is None
    a = fg.VisibleRows(torch.zeros(3, dtype=torch.int32), 3, None, 10)
    b = fg.VisibleRows(torch.zeros(2, dtype=torch.int32), 2, None, 10)
    with fg.appearance_rows(a) as got:
        assert got is a and fg.current_appearance_rows() is a
        with fg.appearance_rows(b):
            assert fg.current_appearance_rows() is b
            with fg.appearance_rows(None):
                assert fg.current_appearance_rows() is None
            assert fg.current_appearance_rows() is b
        assert fg.current_appearance_rows() is a
        with pytest.raises(ZeroDivisionError):
            with fg.appearance_rows(b):
                1 / 0
        assert fg.current_appearance_rows() is a
    assert fg.current_appearance_rows() is None
    with pytest.raises(RuntimeError):
        with fg.appearance_rows(torch.zeros(3, dtype=torch.int32)):
            pass
    assert fg.current_appearance_rows() is None
    # thread-local: another thread sees no list
    import threading
    seen = []
    with fg.appearance_rows(a):
        th = threading.Thread(target=lambda: seen.append(fg.current_appearance_rows()))
        th.start()
        th.join()
    assert seen == [None]


def test_rows_parameter_is_off_by_default():
    import inspect
    fg = FG()
    assert inspect.signature(fg.appearance_mlp).parameters["rows"].default is None
    assert inspect.signature(fg.embedding_forward).parameters["rows"].default is None
    assert list(inspect.signature(fg.appearance_mlp).parameters) == ["inputs", "weights", "shared", "out_scale", "max_workgroups", "rows"]


# ---- GPU: compaction -----------------------------------------------------------------------------------------------------------------------
def _flags(P, density, seed):
    g = torch.Generator().manual_seed(seed)
    if density == "none":
        return torch.zeros(P, dtype=torch.bool)
    if density == "all":
        return torch.ones(P, dtype=torch.bool)
    if density == "alternating":
        return (torch.arange(P) % 2) == 1
    return torch.rand(P, generator=g) < 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["radii", "mask"])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 255, 256, 257, 5000])
def test_compaction_equals_nonzero(P, kind):
    fg = FG()
    f = fg._lib.wg_appearance_rows_compact
    GUARD, SENT = 64, -7
    for di, density in enumerate(("none", "all", "alternating", "random30")):
        on = _flags(P, density, 1000 + P + di)
        g = torch.Generator().manual_seed(P + di)
        if kind == "radii":   # listed iff > 0: unlisted rows hold zeros and negatives
            vals = torch.where(on, torch.randint(1, 400, (P,), generator=g), -torch.randint(0, 3, (P,), generator=g)).to(torch.int32).cuda()
        else:                 # listed iff non-zero: any non-zero byte
            vals = torch.where(on, torch.randint(1, 256, (P,), generator=g), torch.zeros(P, dtype=torch.int64)).to(torch.uint8).cuda()
        want = on.nonzero().reshape(-1).to(torch.int32).cuda()
        nbytes = fg._lib.wg_appearance_rows_compact_scratch_bytes(P)
        got = []
        for _ in range(2):
            rows = torch.full((P + GUARD,), SENT, dtype=torch.int32, device="cuda")
            count = torch.full((1 + GUARD,), SENT, dtype=torch.int32, device="cuda")
            scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            ptr = vals.data_ptr() if P else None
            st = f(P, ptr if kind == "radii" else None, ptr if kind == "mask" else None, rows.data_ptr() if P else None, count.data_ptr(),
                   scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
            assert st == 0
            n = int(count[0])
            assert n == want.numel(), (P, density, n)
            assert torch.equal(rows[:n], want), (P, density)
            assert bool((rows[n:] == SENT).all()) and bool((count[1:] == SENT).all()), (P, density)   # rows[count..P) and the guard behind rows[P]
            got.append(rows)
        assert torch.equal(got[0], got[1])
        # the Python front: no synchronisation is needed to build it, the capacity is P and the count lives on the device
        vr = fg.VisibleRows.from_radii(vals) if kind == "radii" else fg.VisibleRows.from_mask(on.cuda() if di % 2 else vals)
        assert vr.M == P and vr.P == P and vr.count.dtype == torch.int32 and vr.count.is_cuda
        assert int(vr.count[0]) == want.numel() and torch.equal(vr.index[:want.numel()], want)


# ---- GPU: the operator ---------------------------------------------------------------------------------------------------------------------
def _run(c, cot, per_row, colour_view, max_workgroups, rows=None):
    """appearance_mlp forward + backward on the device -> dict with out, dx (colour | gemb [| aemb rows]), dshared, dW1..db3."""
    fg = FG()
    dev = "cuda"
    feats = c["features"].to(dev)
    colour = (feats[:, :3] if colour_view else feats[:, :3].contiguous()).detach().requires_grad_(True)
    gemb = c["gemb"].to(dev).requires_grad_(True)
    W = [w.to(dev).requires_grad_(True) for w in c["weights"]]
    P = feats.shape[0]
    if per_row:
        aemb = c["aemb"][None].repeat(P, 1).to(dev).requires_grad_(True)
        out = fg.appearance_mlp((colour, gemb, aemb), W, max_workgroups=max_workgroups, rows=rows)
    else:
        aemb = c["aemb"].to(dev).requires_grad_(True)
        out = fg.appearance_mlp((colour, gemb), W, shared=aemb, max_workgroups=max_workgroups, rows=rows)
    assert out.shape == (P, 6) and out.dtype == torch.float32
    out.backward(cot.to(dev))
    r = {"out": out.detach(), "dx": torch.cat([colour.grad, gemb.grad] + ([aemb.grad] if per_row else []), 1)}
    if not per_row:
        r["dshared"] = aemb.grad
    for n, w in zip(WNAMES, W):
        r[n] = w.grad
    return r


def _gathered(c, idx):
    """Case c with its per-row tensors gathered by idx (a CPU int64 tensor)."""
    g = dict(c)
    g["features"], g["gemb"], g["P"] = c["features"][idx].contiguous(), c["gemb"][idx].contiguous(), int(idx.numel())
    return g


def _assert_same_bits(r, d, idx, P, tag):
    """r: the rows operator over all P rows; d: the dense operator on the gathered inputs."""
    dev_idx = idx.cuda()
    unlisted = torch.ones(P, dtype=torch.bool, device="cuda")
    unlisted[dev_idx] = False
    for k in ("out", "dx"):
        assert torch.equal(r[k][dev_idx], d[k]), (tag, k)
        assert bool((r[k][unlisted] == 0).all()), (tag, k, "unlisted rows")
    for k in r:
        if k not in ("out", "dx"):
            assert torch.equal(r[k], d[k]), (tag, k)


def _list(P, M, seed, shuffled):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(P, generator=g)[:M]
    return idx if shuffled else idx.sort().values


@pytest.mark.gpu
@pytest.mark.parametrize("M", [0, 1, 31, 32, 33, 63, 64, 65, 129, 200])
def test_bit_identity_with_the_dense_operator_on_gathered_inputs(M):
    fg = FG()
    c = case(*CASE)
    P = c["P"]
    cot = L.dense_cotangent(P, CASE[3])
    for shuffled in (False, True):
        idx = _list(P, M, 7 + M, shuffled)
        rows = fg.VisibleRows.from_index(idx.cuda(), P)
        assert rows.M == M and rows.count is None
        for per_row in (False, True):
            for wgs in (2, 3):
                dense = _run(_gathered(c, idx), cot[idx], per_row, True, wgs)
                for colour_view in (True, False):
                    r = _run(c, cot, per_row, colour_view, wgs, rows=rows)
                    _assert_same_bits(r, dense, idx, P, f"M={M} shuffled={shuffled} per_row={per_row} wgs={wgs} view={colour_view}")


@pytest.mark.gpu
@pytest.mark.parametrize("density", ["none", "random30", "all"])
def test_device_count_and_host_count_give_the_same_bits(density):
    fg = FG()
    c = case(*CASE)
    P = c["P"]
    cot = L.dense_cotangent(P, CASE[3])
    on = _flags(P, density, 99)
    radii = torch.where(on, torch.full((P,), 5), torch.full((P,), -1)).to(torch.int32).cuda()
    dev_rows = fg.VisibleRows.from_radii(radii)
    host_rows = fg.VisibleRows.from_index(on.nonzero().reshape(-1).cuda(), P)
    assert dev_rows.M == P and dev_rows.count is not None and host_rows.M == int(on.sum()) and host_rows.count is None
    for per_row in (False, True):
        a = _run(c, cot, per_row, True, 3, rows=dev_rows)
        b = _run(c, cot, per_row, True, 3, rows=host_rows)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (density, per_row, k)
        if density == "none":
            assert all(bool((a[k] == 0).all()) for k in a)   # an empty list: zeros everywhere, weight gradients and dshared included


def _raw(c, index, M, count, cot, max_workgroups=3, guard=256, sentinel=-12345.0):
    """Forward and backward at the C-ABI over sentinel-filled buffers with guard floats on both sides -> (out, g_colour, g_gemb, dshared, weight
    gradients, all_guards_intact)."""
    fg = FG()
    dev = "cuda"
    P = c["P"]
    feats, gemb, aemb = c["features"].to(dev), c["gemb"].to(dev), c["aemb"].to(dev)
    W = [w.to(dev) for w in c["weights"]]
    g = cot.to(dev).contiguous()

    def guarded(n):
        return torch.full((guard + n + guard,), sentinel, device=dev)
    bufs = {"out": guarded(P * 6), "g0": guarded(P * 3), "g1": guarded(P * c["G"]), "gsh": guarded(c["E"])}
    a = fg._RowsArgs()
    fg._mlp_fill(a.mlp, [feats[:, :3], gemb], aemb, W, 0.01, max_workgroups, torch.cuda.current_stream().cuda_stream)
    a.struct_size = C.sizeof(fg._RowsArgs)
    a.rows, a.M, a.rows_count = index.data_ptr(), M, (None if count is None else count.data_ptr())
    m = a.mlp
    m.out = bufs["out"][guard:].data_ptr()
    assert fg._lib.wg_appearance_rows_forward(C.byref(a)) == 0
    m.dL_dout = g.data_ptr()
    m.grad_segment[0], m.grad_row_stride[0] = bufs["g0"][guard:].data_ptr(), 3
    m.grad_segment[1], m.grad_row_stride[1] = bufs["g1"][guard:].data_ptr(), c["G"]
    m.grad_shared = bufs["gsh"][guard:].data_ptr()
    gw = [torch.full_like(w, sentinel) for w in W]
    m.dW1, m.db1, m.dW2, m.db2, m.dW3, m.db3 = [x.data_ptr() for x in gw]
    n = fg.appearance_rows_scratch_floats(M, max_workgroups)
    scratch = torch.empty(n, device=dev)
    m.scratch, m.scratch_floats = scratch.data_ptr(), n
    assert fg._lib.wg_appearance_rows_backward(C.byref(a)) == 0
    torch.cuda.synchronize()
    intact = all(bool((b[:guard] == sentinel).all()) and bool((b[-guard:] == sentinel).all()) for b in bufs.values())
    body = lambda k, w: bufs[k][guard:-guard].view(P, w)   # noqa: E731
    return body("out", 6), body("g0", 3), body("g1", c["G"]), bufs["gsh"][guard:-guard], gw, intact


@pytest.mark.gpu
def test_out_of_range_entries_are_skipped_and_contribute_exact_zeros():
    c = case(*CASE)
    P = c["P"]
    SENT = -12345.0
    cot = L.dense_cotangent(P, CASE[3])
    valid = _list(P, 66, 5, True)                       # 70 entries: two tiles, the second ragged
    entries = valid.tolist()
    for at, bad in ((3, -1), (31, P), (40, 2 ** 31 - 1), (68, -1)):
        entries.insert(at, bad)
    index = torch.tensor(entries, dtype=torch.int64)
    ok = (index >= 0) & (index < P)
    assert int((~ok).sum()) == 4 and index.numel() == 70
    # the dense run on gathered inputs in which the bad slots hold a valid row (row 0) under a zero cotangent
    stand_in = torch.where(ok, index, torch.zeros_like(index))
    dense = _run(_gathered(c, stand_in), torch.where(ok[:, None], cot[stand_in], torch.zeros(())), False, True, 3)
    out, g0, g1, gsh, gw, intact = _raw(c, index.to(torch.int32).cuda(), 70, None, cot, sentinel=SENT)
    assert intact
    listed = index[ok].cuda()
    okd = ok.cuda()
    assert torch.equal(out[listed], dense["out"][okd])
    assert torch.equal(torch.cat([g0, g1], 1)[listed], dense["dx"][okd])
    assert torch.equal(gsh, dense["dshared"])
    for n, g in zip(WNAMES, gw):
        assert torch.equal(g, dense[n]), n
    unlisted = torch.ones(P, dtype=torch.bool, device="cuda")
    unlisted[listed] = False
    for buf in (out, g0, g1):
        assert bool((buf[unlisted] == SENT).all())      # unlisted rows keep their sentinel: nothing but listed rows is written


@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [True, False], ids=["aemb-per-row", "aemb-shared"])
def test_float64_oracle(per_row):
    fg = FG()
    c = case(*CASE)
    P = c["P"]
    listed = _flags(P, "random30", 11) | _flags(P, "alternating", 0)
    cot = L.dense_cotangent(P, CASE[3])
    o = L.oracle(c, cot * listed[:, None])
    r = _run(c, cot, per_row, True, 3, rows=fg.VisibleRows.from_mask(listed.cuda()))
    Kr = r["dx"].shape[1]
    q = L.ratio(r["out"][listed.cuda()], o["out"][listed], o["e_out"][listed])
    print(f"out (listed rows): max err/bound {q:.3f}")
    assert q <= 1.0
    for k in ["dx"] + WNAMES + ([] if per_row else ["dshared"]):
        want, bound = o[k], o["e_" + k]
        if k == "dx":
            want, bound = want[:, :Kr], bound[:, :Kr]
        q = L.ratio(r[k], want, bound)
        print(f"{k}: max err/bound {q:.3f}")
        assert q <= 1.0, (k, q)


def _shared_call(fg, dev, radii, W, need_grad):
    """dev: the case's (features, gemb, aemb) already on the device, so that the call itself copies nothing from the host."""
    colour, gemb = dev[0][:, :3].detach().requires_grad_(need_grad), dev[1].detach().requires_grad_(need_grad)
    aemb = dev[2].detach().requires_grad_(need_grad)
    out = fg.appearance_mlp((colour, gemb), W, shared=aemb, max_workgroups=3, rows=fg.VisibleRows.from_radii(radii))
    return out, (colour, gemb, aemb)


@pytest.mark.gpu
def test_list_and_operator_do_not_synchronise():
    """from_radii, the forward and the backward pass run under torch's synchronisation check set to "error": no host read anywhere."""
    fg = FG()
    c = case(*CASE)
    P = c["P"]
    radii = torch.where(_flags(P, "random30", 3), 7, 0).to(torch.int32).cuda()
    W = [w.cuda().requires_grad_(True) for w in c["weights"]]
    cot = L.dense_cotangent(P, CASE[3]).cuda()
    dev = (c["features"].cuda(), c["gemb"].cuda(), c["aemb"].cuda())
    ref, leaves = _shared_call(fg, dev, radii, W, True)
    ref_grads = torch.autograd.grad(ref, list(leaves) + W, cot)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            float(torch.ones(1, device="cuda").sum())
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got, leaves = _shared_call(fg, dev, radii, W, True)
            got_grads = torch.autograd.grad(got, list(leaves) + W, cot)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not honoured:
        pytest.skip("this torch build does not raise on a synchronising call in sync debug mode 'error'")
    assert torch.equal(got, ref) and all(torch.equal(a, b) for a, b in zip(got_grads, ref_grads))


@pytest.mark.gpu
def test_captured_once_and_replayed_on_other_radii():
    """Compaction and forward captured in ONE graph: a replay reads the count on the device, so it follows the radii of the replay."""
    fg = FG()
    c = case(*CASE)
    P = c["P"]
    first, second = _flags(P, "random30", 3), _flags(P, "alternating", 0)
    radii = torch.where(first, 7, 0).to(torch.int32).cuda()
    W = [w.cuda() for w in c["weights"]]
    dev = (c["features"].cuda(), c["gemb"].cuda(), c["aemb"].cuda())
    other = torch.where(second, 7, 0).to(torch.int32).cuda()
    with torch.no_grad():
        want_first = _shared_call(fg, dev, radii, W, False)[0]
        want_second = _shared_call(fg, dev, other, W, False)[0]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _shared_call(fg, dev, radii, W, False)[0]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_first)
        radii.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
    assert first.sum() != second.sum() and torch.equal(out, want_second)
    assert bool((out[~second.cuda()] == 0).all())


# ---- GPU: with the rasterizer --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_workgroups", [1, 3])
def test_consistency_with_the_rasterizer(max_workgroups):
    """Loss and every parameter gradient of "dense MLP -> toned rasterizer call" equal those of "MLP over the rows that frame's radii list":
    an unlisted row's colour is never read and its cotangent is zero.

    Per-row quantities (the loss, the gradients of features, gembedding and the geometry) do not depend on where a row sits in the walk and
    are compared at both grids.  The weight gradients and the shared embedding's are sums over rows: a workgroup's partial is ONE chain of
    fused multiply-adds over its rows in order, and a zero cotangent adds exact zeros, so with one workgroup the dense sum and the listed sum
    are the same chain and the same bits.  With several workgroups the dense walk deals rows to partials by row number and the list by
    list position, the partials are added in another grouping, and equal bits cannot be expected (they are compared at
    max_workgroups = 1 only; the grouped sums are held to the dense operator on gathered inputs above)."""
    import wg_scenes as S
    from diff_gaussian_rasterization import GaussianRasterizer
    from wg_testlib import make_settings, to_dev
    fg = FG()
    Wd, Hd, P, G, E, DEG = 64, 48, 357, 24, 32, 3
    cam, cot = S.make_camera(Wd, Hd), to_dev(S.make_cotangent(Wd, Hd))
    cloud = S.make_cloud(P, Wd, Hd, sh_degree=DEG, seed=3, scale_mult=4.0)
    rs = make_settings(cam, DEG)
    g = torch.Generator().manual_seed(5)
    gemb0, aemb0 = torch.rand(P, G, generator=g) * 2 - 1, torch.randn(E, generator=g) * 0.3
    weights = L.draw_weights(3 + G + E, 77)
    results = []
    radii_seen = []
    for use_rows in (False, True):
        t = {k: to_dev(v).requires_grad_(True) for k, v in cloud.items() if k != "shs"}
        t["means2D"] = torch.zeros_like(t["means3D"], requires_grad=True)
        feats = to_dev(cloud["shs"]).reshape(P, 48).requires_grad_(True)
        gemb, aemb = gemb0.cuda().requires_grad_(True), aemb0.cuda().requires_grad_(True)
        m = L.load_weights(L.StubEmbedding(3 + G + E), weights, torch.float32, "cuda")
        geom = dict(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
        rows = None
        if use_rows:   # the caller's raw call comes first and returns the frame's radii
            with torch.no_grad():
                _, radii, _ = GaussianRasterizer(rs)(shs=feats.view(P, 16, 3), **geom)
            rows = fg.VisibleRows.from_radii(radii)
        toned = fg.embedding_forward(m, gemb, aemb, feats, max_workgroups=max_workgroups, rows=rows)
        assert m.calls == []
        color, radii, _ = GaussianRasterizer(rs)(shs=toned.view(P, 16, 3), deterministic_backward=True, **geom)
        loss = (color * cot).sum()
        loss.backward()
        radii_seen.append(radii)
        per_row = dict(loss=loss.detach(), features=feats.grad, gemb=gemb.grad, **{k: v.grad for k, v in geom.items()})
        summed = dict(aemb=aemb.grad, **{n: p.grad for n, p in m.named_parameters()})
        results.append((per_row, summed))
    assert torch.equal(radii_seen[0], radii_seen[1])
    n = int((radii_seen[0] > 0).sum())
    assert 0 < n < P, n   # the frame culls some rows and keeps some
    (dr, ds), (rr, rsum) = results
    for k in dr:
        assert dr[k] is not None and torch.equal(dr[k], rr[k]), k
    if max_workgroups == 1:
        assert len(ds) == 7
        for k in ds:
            assert ds[k] is not None and torch.equal(ds[k], rsum[k]), k


# ---- GPU: the module's forward -------------------------------------------------------------------------------------------------------------
def _golden():
    import json
    z = np.load(L.GOLDEN)
    assert [tuple(x) for x in json.loads(str(z["cases"]))] == [tuple(x) for x in L.GOLDEN_CASES]
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["rows=", "context manager"])
@pytest.mark.parametrize("shared", [False, True], ids=["aemb-per-row", "aemb-shared"])
@pytest.mark.parametrize("i", range(len(L.GOLDEN_CASES)))
def test_embedding_forward_over_rows_against_the_fixture(i, shared, how):
    import wg_integration
    fg = FG()
    z = _golden()
    P, G, E, seed = L.GOLDEN_CASES[i]
    c = case(P, G, E, seed)
    r = L.module_oracle(c, L.golden_cot48(P, seed))
    listed = torch.ones(1, dtype=torch.bool) if P == 1 else (torch.arange(P) % 3) != 1
    rows = fg.VisibleRows.from_mask(listed.cuda())
    if how == "rows=":
        m = L.load_weights(L.StubEmbedding(c["K"]), c["weights"], torch.float32, "cuda")
        res = L.run_module(lambda mod, g, a, col: fg.embedding_forward(mod, g, a, col, max_workgroups=3, rows=rows), m, c, not shared, torch.float32, "cuda")
    else:
        class EmbeddingModel(L.StubEmbedding):
            pass
        mod = types.SimpleNamespace(GaussianModel=type("GaussianModel", (), {}), EmbeddingModel=EmbeddingModel)
        undo = wg_integration.apply_optins(mod, appearance_mlp=True, **OFF)
        try:
            m = L.load_weights(EmbeddingModel(c["K"]), c["weights"], torch.float32, "cuda")

            def fwd(model, g, a, col):
                with fg.appearance_rows(rows):
                    return model(g, a, col)
            res = L.run_module(fwd, m, c, not shared, torch.float32, "cuda")
            # a list built for another row count is refused
            with fg.appearance_rows(fg.VisibleRows.from_mask(torch.ones(P + 1, dtype=torch.bool, device="cuda"))):
                with pytest.raises(RuntimeError):
                    m(c["gemb"].cuda(), c["aemb"].cuda(), c["features"].cuda())
        finally:
            undo()
    assert m.calls == []   # the fused path ran, not the module's own forward
    keys = {"toned": "toned", "d_features": "d_features", "d_gemb": "d_gemb"}
    if not shared:
        keys["d_aemb"] = "d_aemb_rows"
    for k, ok in keys.items():   # the per-row results: listed rows within the existing bound, unlisted rows exactly 0
        want, bound = torch.from_numpy(z[f"{k}64_{i}"]), r["e_" + ok]
        got = torch.from_numpy(res[k])
        assert got.shape == want.shape, k
        q = L.ratio(got[listed], want[listed], bound[listed])
        print(f"case {i} shared={shared} {how} {k}: max err/bound {q:.3f}")
        assert q <= 1.0, (k, q)
        assert bool((got[~listed] == 0).all()), k
