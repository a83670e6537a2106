"""The Adam step over a list of rows (include/wg_adam_rows.h, wg_fused_gaussians.VisibleRowsAdam, apply_optins(visible_adam=True)): a listed
row has the bits of the dense kernel (wg_fused_adam) run on gathered copies, an unlisted row keeps the bits of its parameter and both moments
whatever its gradient holds, and the optimizer above it is FusedAdam wherever no list is given."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = {"xyz": 3, "features_dc": 3, "opacities": 1, "scales": 3, "rotations": 4, "embeddings": 24, "features_rest": 45}   # the reference's rows
LRS = {"xyz": 1.6e-4, "features_dc": 2.5e-3, "opacities": 5e-2, "scales": 5e-3, "rotations": 1e-3, "embeddings": 5e-3, "features_rest": 2.5e-3 / 20}
PS = (1, 63, 64, 65, 1000, 2049, 5000)   # 2049 crosses the compaction's 2048-entry block
GUARD, SENT = 256, -12345.0
INVALID = -1   # WG_ERR_INVALID_ARGUMENT
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
RTOL = 2e-6    # tests/test_adam.py's gate for this arithmetic against torch, relative to each array's largest magnitude


def _fg():
    import wg_fused_gaussians as fg
    return fg


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the lists -----------------------------------------------------------------------------------------------------------------------------
def _lists(P, dev):
    """name -> VisibleRows.  The seeded 30 % share comes four ways: compacted from a mask (capacity P, count on the device), as an exact
    ascending list, shuffled, and with out-of-range entries mixed in."""
    fg = _fg()
    g = torch.Generator().manual_seed(100 + P)
    mask = torch.rand(P, generator=g) < 0.3
    share = torch.nonzero(mask).flatten().to(torch.int32)
    shuffled = share[torch.randperm(share.numel(), generator=g)]
    bad = torch.tensor([-1, P, 2 ** 31 - 1], dtype=torch.int32)
    mixed = torch.cat((bad[:1], shuffled[: shuffled.numel() // 2], bad[1:2], shuffled[shuffled.numel() // 2:], bad[2:]))
    idx = lambda t: fg.VisibleRows.from_index(t.to(dev), P)   # noqa: E731
    return {
        "empty": idx(torch.zeros(0, dtype=torch.int32)),
        "all": idx(torch.arange(P, dtype=torch.int32)),
        "first": idx(torch.tensor([0], dtype=torch.int32)),
        "last": idx(torch.tensor([P - 1], dtype=torch.int32)),
        "every_other": idx(torch.arange(0, P, 2, dtype=torch.int32)),
        "share_device_count": fg.VisibleRows.from_mask(mask.to(dev)),
        "share_exact": idx(share),
        "share_shuffled": idx(shuffled),
        "out_of_range": idx(mixed),
    }


def _valid_rows(rows, P):
    """The list's entries inside [0, P), in list order, as int64 (a host read: test code)."""
    n = rows.M if rows.count is None else int(rows.count.item())
    e = rows.index[:n].long()
    return e[(e >= 0) & (e < P)]


# ---- tensors between guard words -------------------------------------------------------------------------------------------------------------
class _Guarded:
    def __init__(self, values):
        self.buf = torch.full((GUARD + values.numel() + GUARD,), SENT, device=values.device)
        self.body = self.buf[GUARD:GUARD + values.numel()].view(values.shape)
        self.body.copy_(values)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[self.buf.numel() - GUARD:] == SENT).all())


def _state(P, dev, seed):
    """name -> (param, grad, exp_avg, exp_avg_sq) [P, width] float32; gradient magnitudes span 1e-6 .. 1 row by row (tests/test_adam.py)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, w in WIDTHS.items():
        mag = 10.0 ** torch.randint(-6, 1, (P, 1), generator=g).float()
        out[name] = tuple(t.to(dev) for t in (torch.randn(P, w, generator=g), torch.randn(P, w, generator=g) * mag,
                                              torch.randn(P, w, generator=g) * mag * 0.1, (torch.randn(P, w, generator=g) * mag) ** 2))
    return out


def _descriptor(p, g, m, v, lr, step, wd):
    return _fg()._AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), BETA2, 1.0 - BETA1, 1.0 - BETA2,
                             lr / (1.0 - BETA1 ** step), (1.0 - BETA2 ** step) ** 0.5, EPS, wd)


def _rows_step(descs_widths, P, rows):
    fg = _fg()
    arr = (fg._AdamRowsTensor * len(descs_widths))(*[fg._AdamRowsTensor(d, w) for d, w in descs_widths])
    return fg._lib.wg_adam_rows_step(len(descs_widths), arr, P, rows.index.data_ptr(), rows.M,
                                     None if rows.count is None else rows.count.data_ptr(), _stream())


def _dense_step(descs):
    fg = _fg()
    arr = (fg._AdamTensor * len(descs))(*descs)
    return fg._lib.wg_fused_adam(len(descs), arr, _stream())


# ---- 1, 2: listed rows have the dense kernel's bits, unlisted rows are untouched -------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
def test_listed_rows_have_the_dense_kernels_bits_and_unlisted_rows_keep_theirs(P):
    dev = torch.device("cuda")
    lists = _lists(P, dev)
    for case, (wd, step) in enumerate(((0.0, 1), (0.01, 1), (0.0, 1000), (0.01, 1000))):
        state = _state(P, dev, seed=7 * P + case)
        for lname, rows in lists.items():
            valid = _valid_rows(rows, P)
            listed = torch.zeros(P, dtype=torch.bool, device=dev)
            listed[valid] = True
            work, gathered, expect = {}, {}, {}
            for name, (p, g, m, v) in state.items():
                g = g.clone()
                g[~listed] = float("nan")   # the gradient of an unlisted row is never used
                work[name] = (_Guarded(p), _Guarded(g), _Guarded(m), _Guarded(v))
                gathered[name] = tuple(t[valid].contiguous() for t in (p, g, m, v))   # x[rows], in list order
            assert _dense_step([_descriptor(*gathered[n], LRS[n], step, wd) for n in WIDTHS]) == 0   # the existing kernel on the copies
            for name, (p, g, m, v) in state.items():
                expect[name] = []
                for before, after in zip((p, m, v), (gathered[name][0], gathered[name][2], gathered[name][3])):
                    e = before.clone()
                    e[valid] = after
                    expect[name].append(e)
            status = _rows_step([(_descriptor(*(t.body for t in work[n]), LRS[n], step, wd), WIDTHS[n]) for n in WIDTHS], P, rows)
            assert status == 0, (lname, status)
            for name in WIDTHS:
                gp, gg, gm, gv = work[name]
                for what, got, want in zip(("param", "exp_avg", "exp_avg_sq"), (gp, gm, gv), expect[name]):
                    # one comparison of all bits: the dense kernel's at the listed rows, the state before the call everywhere else
                    assert torch.equal(_bits(got.body), _bits(want)), (P, lname, wd, step, name, what)
                assert all(t.intact() for t in (gp, gg, gm, gv)), (P, lname, name, "guard words")
            if valid.numel() and valid.numel() < P:   # the comparison above did cover rows of both kinds
                p0 = state["embeddings"][0]
                assert not torch.equal(work["embeddings"][0].body[valid], p0[valid])
                assert torch.equal(_bits(work["embeddings"][0].body[~listed]), _bits(p0[~listed]))


def test_an_exact_list_and_a_device_count_with_capacity_P_give_the_same_bits():
    dev = torch.device("cuda")
    P = 2049
    lists = _lists(P, dev)
    assert lists["share_device_count"].count is not None and lists["share_device_count"].M == P and lists["share_exact"].count is None
    results = []
    for rows in (lists["share_device_count"], lists["share_exact"], lists["share_shuffled"]):
        state = {n: tuple(t.clone() for t in ts) for n, ts in _state(P, dev, seed=3).items()}
        assert _rows_step([(_descriptor(*state[n], LRS[n], 3, 0.01), WIDTHS[n]) for n in WIDTHS], P, rows) == 0
        results.append(state)
    for other in results[1:]:
        for n in WIDTHS:
            for a, b in zip(results[0][n], other[n]):
                assert torch.equal(_bits(a), _bits(b)), n


# ---- 3, 4, 5: the optimizer --------------------------------------------------------------------------------------------------------------------
def _groups(dev, seed=0, n=1000):
    """tests/test_adam.py's groups: the seven per-Gaussian ones and the dense ones (per-image embeddings with weight decay, MLP shapes with
    ragged tails)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda *shape: torch.nn.Parameter(torch.randn(*shape, generator=g).to(dev))   # noqa: E731
    return [
        {"params": [mk(n, 3)], "lr": 1.6e-4, "name": "xyz"},
        {"params": [mk(n, 1, 3)], "lr": 2.5e-3, "name": "features_dc"},
        {"params": [mk(n, 1)], "lr": 5e-2, "name": "opacities"},
        {"params": [mk(n, 3)], "lr": 5e-3, "name": "scales"},
        {"params": [mk(n, 4)], "lr": 1e-3, "name": "rotations"},
        {"params": [mk(7, 32)], "lr": 1e-3, "name": "appearance_embeddings", "weight_decay": 0.01},
        {"params": [mk(n, 24)], "lr": 5e-3, "name": "embeddings"},
        {"params": [mk(n, 15, 3)], "lr": 2.5e-3 / 20, "name": "features_rest"},
        {"params": [mk(64, 67), mk(64), mk(13), mk(1)], "lr": 5e-4, "name": "appearance_mlp"},
    ]


def _twin(groups, cls, **kw):
    copies = copy.deepcopy(groups)
    for a, b in zip(groups, copies):
        b["params"] = [torch.nn.Parameter(p.detach().clone()) for p in a["params"]]
    return cls(copies, lr=1.0, eps=1e-15, **kw)


def _set_grads(optimizers, step, skip=()):
    g = torch.Generator(device="cpu").manual_seed(1000 + step)
    for groups in zip(*(o.param_groups for o in optimizers)):
        for params in zip(*(gr["params"] for gr in groups)):
            if groups[0]["name"] in skip:
                for p in params:
                    p.grad = None
                continue
            gr = (torch.randn(params[0].shape, generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))).to(params[0].device)
            for p in params:
                p.grad = gr.clone()


def _all(optimizer):
    """[(group name, what, tensor)] of every parameter and moment."""
    out = []
    for gr in optimizer.param_groups:
        for k, p in enumerate(gr["params"]):
            st = optimizer.state.get(p, {})
            out.append((gr["name"], f"param{k}", p.detach()))
            out += [(gr["name"], f"{key}{k}", st[key]) for key in ("exp_avg", "exp_avg_sq") if key in st]
    return out


def _assert_equal(a, b, what=""):
    ta, tb = _all(a), _all(b)
    assert [x[:2] for x in ta] == [x[:2] for x in tb], what
    for (name, key, x), (_, _, y) in zip(ta, tb):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, name, key)
    for ga, gb in zip(a.param_groups, b.param_groups):
        for pa, pb in zip(ga["params"], gb["params"]):
            assert float(a.state[pa]["step"]) == float(b.state[pb]["step"]) if pa in a.state else pb not in b.state, (what, ga["name"], "step")


def _assert_close(a, b, what=""):
    for (name, key, x), (_, _, y) in zip(_all(a), _all(b)):
        assert float((x - y).abs().max()) <= RTOL * (float(x.abs().max()) + 1e-30), (what, name, key)


def test_every_row_listed_is_fused_adam_bit_for_bit():
    fg = _fg()
    dev = torch.device("cuda")
    groups = _groups(dev)
    dense, sparse = _twin(groups, fg.FusedAdam), _twin(groups, fg.VisibleRowsAdam)
    P = 1000
    for step in range(10):
        if step == 5:   # the learning-rate schedule writes the group's lr
            for o in (dense, sparse):
                o.param_groups[0]["lr"] = 3.1e-5
        _set_grads((dense, sparse), step)
        dense.step()
        if step % 3 == 0:
            sparse.visible(torch.ones(P, dtype=torch.int32, device=dev))   # radii: compacted on the device, the count stays there
            sparse.step()
        elif step % 3 == 1:
            sparse.step(rows=fg.VisibleRows.from_index(torch.arange(P, device=dev), P))
        else:
            sparse.step(rows=fg.VisibleRows.from_mask(torch.ones(P, dtype=torch.bool, device=dev)))
        _assert_equal(dense, sparse, f"step {step}")
    assert sparse.row_steps == 10 and sparse.dense_steps == 0


def test_changing_visibility_follows_torch_adam_on_the_gathered_rows():
    """Twenty steps, a fresh seeded mask each: the reference is torch.optim.Adam itself stepping the gathered rows (its state seeded with the
    gathered moments and the GLOBAL step count), copied back.  Row 7 is unlisted for the first ten steps and has its initial bits then."""
    fg = _fg()
    dev = torch.device("cuda")
    P = 1000
    groups = [g for g in _groups(dev, seed=11, n=P) if g["name"] in WIDTHS or g["name"] == "appearance_embeddings"]
    sparse = _twin(groups, fg.VisibleRowsAdam)
    ref = {g["name"]: [g["params"][0].detach().clone(), torch.zeros_like(g["params"][0]), torch.zeros_like(g["params"][0])] for g in groups}
    initial = {g["name"]: g["params"][0].detach().clone() for g in groups}
    gen = torch.Generator().manual_seed(5)
    for step in range(20):
        mask = torch.rand(P, generator=gen) < 0.4
        if step < 10:
            mask[7] = False
        mask = mask.to(dev)
        idx = torch.nonzero(mask).flatten()
        _set_grads((sparse,), step)
        for g in sparse.param_groups:
            name, grad = g["name"], g["params"][0].grad
            sel = idx if name in WIDTHS else torch.arange(grad.shape[0], device=dev)   # the dense group: every row, every step
            p = torch.nn.Parameter(ref[name][0][sel].clone())
            o = torch.optim.Adam([p], lr=g["lr"], eps=1e-15, weight_decay=g.get("weight_decay", 0), foreach=False)
            o.state[p] = {"step": torch.tensor(float(step)), "exp_avg": ref[name][1][sel].clone(), "exp_avg_sq": ref[name][2][sel].clone()}
            p.grad = grad[sel].clone()
            o.step()
            ref[name][0][sel], ref[name][1][sel], ref[name][2][sel] = p.detach(), o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"]
        sparse.visible(fg.VisibleRows.from_mask(mask))
        sparse.step()
        if step == 9:
            for g in sparse.param_groups:
                if g["name"] in WIDTHS:
                    p = g["params"][0]
                    assert torch.equal(_bits(p.detach()[7]), _bits(initial[g["name"]][7])), g["name"]
                    assert not bool(sparse.state[p]["exp_avg"][7].any()) and not bool(sparse.state[p]["exp_avg_sq"][7].any())
        if step in (0, 9, 19):
            for g in sparse.param_groups:
                p = g["params"][0]
                for what, got, want in zip(("param", "exp_avg", "exp_avg_sq"), (p.detach(), sparse.state[p]["exp_avg"], sparse.state[p]["exp_avg_sq"]),
                                           ref[g["name"]]):
                    err, scale = float((got - want).abs().max()), float(want.abs().max()) + 1e-30
                    assert err <= RTOL * scale, (step, g["name"], what, err / scale)
                assert float(sparse.state[p]["step"]) == step + 1   # the global count
    assert sparse.row_steps == 20


def test_the_list_lasts_one_step_and_a_stale_one_is_refused_before_anything_moves():
    fg = _fg()
    dev = torch.device("cuda")
    P = 500
    groups = _groups(dev, seed=2, n=P)
    dense, sparse = _twin(groups, fg.FusedAdam), _twin(groups, fg.VisibleRowsAdam)
    _set_grads((dense, sparse), 0)
    half = torch.arange(P, device=dev) < P // 2
    sparse.visible(fg.VisibleRows.from_mask(half))
    sparse.step()
    dense.step()
    assert (sparse.row_steps, sparse.dense_steps) == (1, 0) and sparse._pending_rows is None
    for (name, key, x), (_, _, y) in zip(_all(sparse), _all(dense)):
        if name in WIDTHS:   # listed rows: the dense step's bits; unlisted rows: the initial parameter, zero moments
            assert torch.equal(_bits(x[: P // 2]), _bits(y[: P // 2])), (name, key)
            start = next(g for g in groups if g["name"] == name)["params"][0].detach() if key.startswith("param") else torch.zeros_like(x)
            assert torch.equal(_bits(x[P // 2:]), _bits(start[P // 2:])), (name, key)
        else:
            assert torch.equal(_bits(x), _bits(y)), (name, key)
    # the next step has no list: dense, and it moves the rows the first one left alone
    before = sparse.param_groups[0]["params"][0].detach().clone()
    _set_grads((sparse,), 1)
    sparse.step()
    assert (sparse.row_steps, sparse.dense_steps) == (1, 1)
    assert bool((sparse.param_groups[0]["params"][0].detach()[P // 2:] != before[P // 2:]).any())
    # a list for another P: refused, nothing launched, no counter moved, the list dropped
    _set_grads((sparse,), 2)
    snapshot = [(n, k, t.clone()) for n, k, t in _all(sparse)]
    steps = [float(sparse.state[p]["step"]) for g in sparse.param_groups for p in g["params"]]
    sparse.visible(torch.ones(P + 3, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match=rf"{P + 3}\D.*\D{P}\D"):
        sparse.step()
    torch.cuda.synchronize()
    for (n, k, a), (_, _, b) in zip(snapshot, _all(sparse)):
        assert torch.equal(_bits(a), _bits(b)), (n, k)
    assert steps == [float(sparse.state[p]["step"]) for g in sparse.param_groups for p in g["params"]]
    assert sparse._pending_rows is None and (sparse.row_steps, sparse.dense_steps) == (1, 1)
    # a per-Gaussian parameter without a gradient is skipped -- before the row-count check -- and its step does not advance
    _set_grads((sparse,), 3, skip=("embeddings",))
    emb = next(g for g in sparse.param_groups if g["name"] == "embeddings")["params"][0]
    emb_before, emb_step = emb.detach().clone(), float(sparse.state[emb]["step"])
    xyz_step = float(sparse.state[sparse.param_groups[0]["params"][0]]["step"])
    sparse.step(rows=fg.VisibleRows.from_mask(half))
    assert torch.equal(_bits(emb.detach()), _bits(emb_before)) and float(sparse.state[emb]["step"]) == emb_step
    assert float(sparse.state[sparse.param_groups[0]["params"][0]]["step"]) == xyz_step + 1
    with pytest.raises(RuntimeError, match="VisibleRows"):
        sparse.visible(torch.ones(P, device=dev))   # float radii: not a list


def test_state_dicts_cross_over_and_the_reference_style_state_surgery_is_followed_by_a_list_for_the_new_P():
    fg = _fg()
    dev = torch.device("cuda")
    groups = _groups(dev, seed=3, n=500)
    ref, dense, sparse = _twin(groups, torch.optim.Adam), _twin(groups, fg.FusedAdam), _twin(groups, fg.VisibleRowsAdam)
    every = lambda n: fg.VisibleRows.from_index(torch.arange(n, device=dev), n)   # noqa: E731
    for step in range(4):
        _set_grads((ref, dense, sparse), step)
        ref.step(), dense.step(), sparse.step(rows=every(500))
    # prune (boolean mask), append (cat), replace (zeros): tests/test_adam.py's second test
    mask = (torch.arange(500, device=dev) % 3) != 0
    for o in (ref, dense, sparse):
        for group in o.param_groups:
            if group["name"] not in WIDTHS:
                continue
            old = group["params"][0]
            st = o.state.get(old)
            ext = torch.full_like(old[:17], 0.25)
            st["exp_avg"] = torch.cat((st["exp_avg"][mask], torch.zeros_like(ext)), dim=0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"][mask], torch.zeros_like(ext)), dim=0)
            del o.state[old]
            group["params"][0] = torch.nn.Parameter(torch.cat((old.detach()[mask], ext), dim=0).requires_grad_(True))
            o.state[group["params"][0]] = st
            if group["name"] == "opacities":
                st["exp_avg"] = torch.zeros_like(group["params"][0])
                st["exp_avg_sq"] = torch.zeros_like(group["params"][0])
    new_P = int(mask.sum()) + 17
    _set_grads((ref, dense, sparse), 4)
    with pytest.raises(RuntimeError, match=rf"500\D.*\D{new_P}\D"):
        sparse.step(rows=every(500))   # the list from before the surgery
    for o in (ref, dense, sparse):
        for group in o.param_groups:
            for p in group["params"]:
                p.grad = None
    for step in range(5, 9):
        _set_grads((ref, dense, sparse), step)
        ref.step(), dense.step(), sparse.step(rows=every(new_P))
    _assert_equal(dense, sparse, "after surgery")
    _assert_close(ref, sparse, "after surgery")
    # state dicts cross over: torch's into the rows optimizer, the rows optimizer's into FusedAdam, FusedAdam's into torch's
    sd_ref, sd_dense, sd_sparse = (copy.deepcopy(o.state_dict()) for o in (ref, dense, sparse))
    sparse.load_state_dict(sd_ref), dense.load_state_dict(sd_sparse), ref.load_state_dict(sd_dense)
    assert isinstance(sparse.per_gaussian, frozenset) and "xyz" in sparse.per_gaussian
    for step in range(9, 12):
        _set_grads((ref, dense, sparse), step)
        ref.step(), dense.step(), sparse.step(rows=every(new_P))
    _assert_close(ref, sparse, "after the state dicts crossed over")
    _assert_close(dense, sparse, "after the state dicts crossed over")
    assert isinstance(sparse, torch.optim.Adam) and isinstance(sparse, fg.FusedAdam)


def test_sixty_one_row_tensors_take_more_than_one_launch():
    fg = _fg()
    dev = torch.device("cuda")
    P = 300
    g = torch.Generator().manual_seed(5)
    widths = [int(torch.randint(1, 50, (1,), generator=g)) for _ in range(61)]   # three launches of <= 24
    pa = [torch.nn.Parameter(torch.randn(P, w, generator=g).to(dev)) for w in widths]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    start = [p.detach().clone() for p in pa]
    dense = fg.FusedAdam([{"params": pa, "name": "xyz"}], lr=1e-2, weight_decay=0.1)
    sparse = fg.VisibleRowsAdam([{"params": pb, "name": "xyz"}], lr=1e-2, weight_decay=0.1)
    mask = torch.rand(P, generator=g) < 0.5
    for a, b in zip(pa, pb):
        a.grad = torch.randn(a.shape, generator=g).to(dev)
        b.grad = a.grad.clone()
    dense.step()
    sparse.step(rows=fg.VisibleRows.from_mask(mask.to(dev)))
    mask = mask.to(dev)
    for a, b, s in zip(pa, pb, start):
        assert torch.equal(_bits(b.detach()[mask]), _bits(a.detach()[mask])) and torch.equal(_bits(b.detach()[~mask]), _bits(s[~mask]))
        assert torch.equal(_bits(sparse.state[b]["exp_avg_sq"][mask]), _bits(dense.state[a]["exp_avg_sq"][mask]))
        assert not bool(sparse.state[b]["exp_avg"][~mask].any())


# ---- 6: the C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_malformed_calls_are_refused_and_empty_ones_return_ok_with_the_arrays_unchanged():
    fg = _fg()
    dev = torch.device("cuda")
    P, w = 100, 4
    p, g, m, v = (torch.randn(P, w, device=dev) for _ in range(4))
    v = v.abs()
    before = [t.clone() for t in (p, m, v)]
    rows = fg.VisibleRows.from_index(torch.arange(P, device=dev), P)
    good = lambda: _descriptor(p, g, m, v, 1e-2, 1, 0.0)   # noqa: E731

    def call(desc=None, width=w, P_=P, rows_ptr=rows.index.data_ptr(), M=P, count_ptr=None, n=1, null_array=False):
        arr = (fg._AdamRowsTensor * 1)(fg._AdamRowsTensor(desc if desc is not None else good(), width))
        return fg._lib.wg_adam_rows_step(n, None if null_array else arr, P_, rows_ptr, M, count_ptr, _stream())

    def with_field(**kw):
        d = good()
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    refused = {
        "null param": call(with_field(param=None)), "null grad": call(with_field(grad=None)),
        "null exp_avg": call(with_field(exp_avg=None)), "null exp_avg_sq": call(with_field(exp_avg_sq=None)),
        "numel != P * width": call(with_field(numel=P * w - 1)), "numel for another P": call(P_=P + 1),
        "width 0": call(width=0), "width -4": call(width=-4),
        "P < 0": call(P_=-1), "P > 2^31 - 1": call(P_=2 ** 31),
        "M < 0": call(M=-1), "M > 2^31 - 1": call(M=2 ** 31),
        "null rows": call(rows_ptr=None),
        "bias_correction2_sqrt <= 0": call(with_field(bias_correction2_sqrt=0.0)),
        "one_minus_beta1 >= 0.5": call(with_field(one_minus_beta1=0.5)),
        "n_tensors < 0": call(n=-1), "null tensors": call(null_array=True),
    }
    assert all(s == INVALID for s in refused.values()), {k: s for k, s in refused.items() if s != INVALID}
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    assert call(M=0) == 0 and call(M=0, rows_ptr=None) == 0 and call(n=0) == 0
    assert call(count_ptr=zero.data_ptr()) == 0                                                  # the count on the device says 0
    negative, huge = (torch.full((1,), n, dtype=torch.int32, device=dev) for n in (-5, 10 ** 6))
    assert call(count_ptr=negative.data_ptr()) == 0   # clamped to [0, M]
    torch.cuda.synchronize()
    for a, b in zip(before, (p, m, v)):
        assert torch.equal(_bits(a), _bits(b))
    # a count beyond the capacity is clamped to it: the first M = 10 entries, no more
    assert call(M=10, count_ptr=huge.data_ptr()) == 0
    assert bool((p[:10] != before[0][:10]).any(dim=1).all()) and torch.equal(_bits(p[10:]), _bits(before[0][10:]))


def test_a_captured_replay_gives_the_eager_calls_bits():
    fg = _fg()
    dev = torch.device("cuda")
    P = 2049
    rows = _lists(P, dev)["share_device_count"]
    start = _state(P, dev, seed=9)
    eager = {n: tuple(t.clone() for t in ts) for n, ts in start.items()}
    assert _rows_step([(_descriptor(*eager[n], LRS[n], 2, 0.01), WIDTHS[n]) for n in WIDTHS], P, rows) == 0
    replay = {n: tuple(t.clone() for t in ts) for n, ts in start.items()}
    descs = [(_descriptor(*replay[n], LRS[n], 2, 0.01), WIDTHS[n]) for n in WIDTHS]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):   # one stream, one native call: no allocation, no host wait inside
            assert _rows_step(descs, P, rows) == 0
        for n, ts in start.items():   # capture ran nothing; start the replay from the same state
            for dst, src in zip(replay[n], ts):
                dst.copy_(src)
        graph.replay()
    stream.synchronize()
    torch.cuda.synchronize()
    for n in WIDTHS:
        for a, b in zip(eager[n], replay[n]):
            assert torch.equal(_bits(a), _bits(b)), n


# ---- 7: the caller's loop ----------------------------------------------------------------------------------------------------------------------
def test_the_callers_training_loop_steps_only_the_gaussians_each_frame_reached():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "real_caller"))
    import harness
    import wg_integration
    fg = _fg()
    m = harness.import_restated()
    GM = m.GaussianModel
    swapped = lambda: (GM._render_internal, GM._setup_optimizers, GM.get_gaussians, GM.add_densification_stats, m.ssim, m.eval_sh)   # noqa: E731
    originals = swapped()
    with pytest.raises(ValueError):
        wg_integration.apply_optins(m, adam=False, visible_adam=True)
    assert swapped() == originals   # refused before anything was swapped
    undo = wg_integration.apply_optins(m, visible_adam=True)
    try:
        m, wg = harness.make_caller(30_000, 480, 320, n_cams=3, overrides={
            "densify_from_iter": 10, "densification_interval": 15, "opacity_reset_interval": 40, "densify_until_iter": 55,
            "densify_grad_threshold": 0.00002})
        model = wg.model
        opt = model.optimizer
        assert type(opt) is fg.VisibleRowsAdam and m.GaussianModel._render_internal is not originals[0]
        handed = []
        visible = opt.visible
        opt.visible = lambda rows: (handed.append(rows), visible(rows))[1]
        counts, losses = [], []
        for i in range(60):
            watched = i == 20   # an iteration without densification (those are 15, 30, 45) or opacity reset (40)
            if watched:
                names = list(m.GaussianModel.PARAMS)
                before = {n: [getattr(model, n).detach().clone()] + [opt.state[getattr(model, n)][k].clone() for k in ("exp_avg", "exp_avg_sq")]
                          for n in names}
            out = wg.train_iteration(i)
            assert opt._pending_rows is None, i   # no list survives an iteration
            if watched:
                radii = handed[-1]
                hidden, seen = radii == 0, radii > 0
                assert bool(hidden.any()) and bool(seen.any())
                changed = torch.zeros_like(seen)
                for n in names:
                    p = getattr(model, n)
                    after = [p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
                    for a, b in zip(before[n], after):
                        assert torch.equal(_bits(a[hidden]), _bits(b[hidden])), n
                        changed |= (a != b).flatten(1).any(dim=1)
                assert bool(changed[seen].any()) and not bool(changed[hidden].any())
            counts.append(out["num_gaussians"])
            losses.append(out["loss"])
        assert np.isfinite(losses).all() and len(set(counts)) > 2
        assert len(handed) == 60 and opt.row_steps > 0 and opt.row_steps + opt.dense_steps == 60
        for p in (model.xyz, model.scales, model.rotations, model.opacities, model.features_dc):
            assert torch.isfinite(p).all() and p.shape[0] == counts[-1]
        # an evaluation render hands over no list
        model.eval()
        wg.render(wg.train_cameras[0], embedding=None)
        assert len(handed) == 60 and opt._pending_rows is None
        with torch.no_grad():   # nor does a training-mode render without grad mode
            model.train()
            wg.render(wg.train_cameras[0], embedding=None)
        assert len(handed) == 60 and opt._pending_rows is None
    finally:
        undo()
    assert swapped() == originals
