"""Device-resident training frames (include/wg_frames.h, wg_frame_store, wg_integration.keep_training_frames_on_device) against what the
reference's training step fetches: `self.train_images[i].to(device)`, `self.train_masks[i].to(device)` (wildgaussians/method.py:1917-1918
over the lists of :1716-1723) and `self._images_cache[key].to(device)` (:264).

Oracle: the host tensor itself.  The store's contract is equality of BITS with `host.to(device)`, so no tolerance appears anywhere: an 8-bit
frame is (float)byte / 255.0f, one correctly rounded float32 division, which tests/golden/frame_store_ref.npz (recorded from the reference's
own convert_image_dtype) pins to NumPy's `astype(np.float32) / 255.0`; everything else is served from a float32 copy.

The fixture's "image_u8" case is 5 x 7 pixels, so each of its channels holds a 35-value stretch of the byte cycle; "image_u8_all" (16 x 16)
and the all-values test below hold all 256 values in every channel.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frame_store_lib as L  # noqa: E402

REFERENCE = "/root/reference"
DEV = "cuda:0"
gpu = pytest.mark.gpu


def bits(t):
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).view(np.uint32)
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def golden():
    z = np.load(L.GOLDEN)
    return {k: z[k] for k in z.files}


def strides(a):
    """Strides in elements of the axes longer than 1 (a length-1 axis has no stride to speak of: NumPy's `[None]` gives it 0)."""
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    return tuple(s for s, n in zip(t.stride(), t.shape) if n > 1)


def recorded(golden, name):
    return L.from_memory_order(golden[name + "_storage"], golden[name + "_perm"])


def host_lists():
    """(train_images, train_masks) as the reference builds them, from the fixture's inputs."""
    inp = L.inputs()
    images = [torch.from_numpy(L.image_array(L.restated_convert, inp[n])) for n in L.IMAGE_CASES]
    masks = [torch.from_numpy(L.mask_array(L.restated_convert, inp[n])) for n in L.MASK_CASES]
    return images, masks


# =============================================================================================== CPU
def test_fixture_is_small_and_holds_every_case(golden):
    assert os.path.getsize(L.GOLDEN) <= 64 * 1024
    inp = L.inputs()
    for name in L.CASES:
        assert np.array_equal(golden[name + "_in"], inp[name]) and golden[name + "_in"].dtype == inp[name].dtype, name
        assert recorded(golden, name).dtype == np.float32
    for c in range(3):
        assert len(set(inp["image_u8_all"][..., c].ravel().tolist())) == 256
    assert set(inp["mask_u8"].ravel().tolist()) - {0, 255}


@pytest.mark.parametrize("name", ["image_u8", "image_u8_all", "mask_u8"])
def test_recorded_uint8_cases_are_one_float32_division(golden, name):
    """The oracle of every GPU test below: astype(np.float32) / 255.0, with the reference's shape and strides."""
    rec = recorded(golden, name)
    mine = L.build_array(lambda img, dtype: img.astype(np.float32) / 255.0, name, golden[name + "_in"])
    assert rec.shape == mine.shape and same_bits(rec, mine)
    assert strides(rec) == strides(mine)
    if name in L.IMAGE_CASES:   # a [3, H, W] view of H x W x 3 storage
        H, W = rec.shape[1:]
        assert torch.from_numpy(rec).stride() == (1, 3 * W, 3)


@pytest.mark.parametrize("name", L.CASES)
def test_restated_list_expressions_reproduce_the_recording(golden, name):
    mine = L.build_array(L.restated_convert, name, golden[name + "_in"])
    assert same_bits(recorded(golden, name), mine)


def test_recording_equals_the_reference_function_where_the_checkout_exists(golden):
    if not os.path.exists(os.path.join(REFERENCE, "wildgaussians", "method.py")):
        pytest.skip("reference checkout not present")
    convert = L.reference_convert(REFERENCE)
    for name in L.CASES:
        fresh = L.build_array(convert, name, golden[name + "_in"])
        rec = recorded(golden, name)
        assert fresh.dtype == np.float32 and same_bits(rec, fresh), name
        assert strides(rec) == strides(fresh), name


def test_a_reciprocal_multiply_is_wrong_for_126_byte_values():
    """Why the kernel divides: byte * (1 / 255) in float32 differs from byte / 255 for 126 of the 256 values."""
    b = np.arange(256).astype(np.float32)
    div = b / np.float32(255.0)
    mul = b * (np.float32(1.0) / np.float32(255.0))
    assert int((div.view(np.uint32) != mul.view(np.uint32)).sum()) == 126
    assert same_bits(div, np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0)


def test_plan_residency():
    from wg_frame_store import plan_residency
    assert plan_residency([], 100) == []
    assert plan_residency([1, 2, 3], 0) == [False, False, False]
    assert plan_residency([40, 60], 100) == [True, True]                      # an exact fit
    assert plan_residency([40, 61], 100) == [True, False]                     # one entry over the budget
    assert plan_residency([10, 500, 20, 30, 41], 100) == [True, False, True, True, False]   # a large entry refused, later small ones admitted
    assert plan_residency([0, 0], 0) == [True, True]


def test_c_abi_refuses_invalid_arguments_before_any_device_work():
    import wg_frame_store as FS
    lib, p = FS._lib, C.c_void_p(64)   # never dereferenced: every call below is refused on its arguments
    assert lib.wg_frames_pack_scratch_words(0) == 0 and lib.wg_frames_pack_scratch_words(1 << 32) == 0
    assert lib.wg_frames_pack_scratch_words(1) == 2 and lib.wg_frames_pack_scratch_words(257) == 3
    assert lib.wg_frames_pack_scratch_words(256 * 8192 * 5) == 8193   # the grid is capped; larger frames stride
    for args in ((0, p, p, p), (8, None, p, p), (8, p, None, p), (8, p, p, None), (1 << 32, p, p, p), (8, C.c_void_p(66), p, p)):
        assert lib.wg_frames_pack(*args, None) == -1, args
    for args in ((0, 8, 1, p, p), (5, 8, 1, p, p), (3, 0, 1, p, p), (3, 8, 1, None, p), (3, 8, 0, p, None), (3, 1 << 30, 1, p, p),
                 (3, 8, 1, p, C.c_void_p(66))):
        assert lib.wg_frames_unpack(*args, None) == -1, args


def test_uncovered_tensors_pass_through_without_touching_the_device():
    from wg_frame_store import FeatureCache, FrameList
    f64 = torch.zeros(3, 4, 5, dtype=torch.float64)
    five = torch.zeros(5, 4, 5)
    flat = torch.zeros(20)
    odd_order = torch.zeros(5, 3, 4).permute(1, 0, 2)        # dense, but neither planar nor pixel-major
    gappy = torch.zeros(3, 4, 10)[:, :, ::2]                 # not dense
    covered_but_no_budget = torch.zeros(3, 4, 5)
    host = [f64, five, flat, odd_order, gappy, covered_but_no_budget]
    frames = FrameList(host, DEV, 0)
    assert len(frames) == len(host)
    assert all(a is b for a, b in zip(frames, host)) and frames[-1] is host[-1] and frames[1:3] == host[1:3]
    s = frames.stats()
    assert s["host_served"] == len(host) and s["uint8"] == s["float32"] == s["resident_bytes"] == 0
    with pytest.raises(IndexError):
        frames[len(host)]
    assert FrameList([f64, five], DEV).stats()["budget_bytes"] == 0   # nothing to hold: the default budget is not even asked for

    cache = FeatureCache(DEV, 1 << 20)
    cache[("a", (1, 2))] = f64              # not float32: kept as it comes
    cache["n"] = None
    cache[("b", (1, 2))] = torch.zeros(4)   # storing uploads nothing: an entry moves to the device when it is first read
    assert cache[("a", (1, 2))] is f64 and cache["n"] is None and ("a", (1, 2)) in cache and len(cache) == 3
    del cache["n"]
    assert list(cache) == [("a", (1, 2)), ("b", (1, 2))]
    assert cache.stats()["resident"] == 0 and cache.stats()["resident_bytes"] == 0
    no_room = FeatureCache(DEV, 15)         # 16 bytes do not fit 15: the entry is served from the host
    t = torch.zeros(4)
    no_room["k"] = t
    assert no_room["k"] is t and no_room.stats() == {"entries": 1, "resident": 0, "host_served": 1, "resident_bytes": 0, "budget_bytes": 15}


def test_opt_in_swaps_and_restores_on_a_stand_in_trainer_without_masks_or_uncertainty_model():
    import wg_integration
    images = [torch.zeros(3, 4, 5, dtype=torch.float64), torch.zeros(3, 2, 2)]
    trainer = types.SimpleNamespace(train_images=images, train_masks=None, model=types.SimpleNamespace(uncertainty_model=None))
    undo = wg_integration.keep_training_frames_on_device(trainer, device=DEV, max_device_bytes=0)
    from wg_frame_store import FrameList
    assert isinstance(trainer.train_images, FrameList) and trainer.train_images.host is images and trainer.train_masks is None
    assert trainer.train_images[0] is images[0] and trainer.train_images[1] is images[1] and len(trainer.train_images) == 2
    assert undo.masks is None and undo.features is None and undo.stats()["images"]["host_served"] == 2
    undo()
    assert trainer.train_images is images and trainer.train_masks is None and trainer.model.uncertainty_model is None
    undo()   # a second call changes nothing
    assert trainer.train_images is images


# =============================================================================================== GPU
SIZES = [(1, 1), (1, 5), (3, 2), (5, 7), (2, 2), (16, 16), (33, 17)]   # HW % 4 = 1, 1, 2, 3, 0, 0, 1; up to three workgroups, ragged
LAYOUTS = [("interleaved", 3), ("interleaved", 1), ("planar", 3)]
SENTINEL = 0x7fc12345   # a NaN with a payload: no conversion result has these bits


def frame_bytes(H, W, Cn, layout):
    """(the stored bytes as a flat array, the planar float32 [C, H, W] oracle)."""
    hwc = L.cycling_bytes(H, W, Cn)
    planar = np.ascontiguousarray(np.moveaxis(hwc.astype(np.float32) / 255.0, -1, 0))
    stored = hwc if layout == "interleaved" else np.ascontiguousarray(np.moveaxis(hwc, -1, 0))
    return stored.reshape(-1), planar


def guarded_unpack(stored, Cn, layout, n, guard, src_shift=0):
    import wg_frame_store as FS
    src = torch.zeros(stored.size + src_shift, dtype=torch.uint8, device=DEV)
    src[src_shift:] = torch.from_numpy(stored.copy()).to(DEV)
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    FS.unpack(src[src_shift:], Cn, layout == "interleaved", out=buf[guard:guard + n])
    torch.cuda.synchronize()
    raw = buf.view(torch.int32).cpu().numpy()
    assert (raw[:guard] == SENTINEL).all() and (raw[guard + n:] == SENTINEL).all(), "a guard float was written"
    return raw[guard:guard + n].view(np.uint32)


@gpu
@pytest.mark.parametrize("guard", [4, 3], ids=["dst16", "dst4"])   # dst on a 16-byte boundary (16-byte stores where HW % 4 == 0) and off it
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("layout,Cn", LAYOUTS)
def test_unpack_equals_the_division_bit_for_bit(golden, layout, Cn, H, W, guard):
    stored, planar = frame_bytes(H, W, Cn, layout)
    got = guarded_unpack(stored, Cn, layout, planar.size, guard)
    assert np.array_equal(got, planar.reshape(-1).view(np.uint32))
    if (H, W, Cn, layout) == (5, 7, 3, "interleaved"):   # the very frame the reference's function was recorded on
        assert np.array_equal(stored.reshape(5, 7, 3), golden["image_u8_in"])
        assert np.array_equal(got.reshape(3, 5, 7), bits(recorded(golden, "image_u8")))


@gpu
@pytest.mark.parametrize("layout,Cn", LAYOUTS + [("interleaved", 2), ("interleaved", 4), ("planar", 4)])
def test_unpack_from_an_odd_source_address(layout, Cn):
    """src one byte off a dword boundary: the byte-load form."""
    stored, planar = frame_bytes(33, 17, Cn, layout)
    got = guarded_unpack(stored, Cn, layout, planar.size, 4, src_shift=1)
    assert np.array_equal(got, planar.reshape(-1).view(np.uint32))


@gpu
@pytest.mark.parametrize("Cn,HW", [(1, 256), (2, 128), (4, 64), (4, 67)])
def test_unpack_all_256_values(Cn, HW):
    import wg_frame_store as FS
    stored = (np.arange(Cn * HW) % 256).astype(np.uint8)
    oracle = stored.astype(np.float32) / 255.0
    for inter in (True, False):
        out = FS.unpack(torch.from_numpy(stored).to(DEV), Cn, inter)
        want = oracle.reshape(HW, Cn).T if inter else oracle.reshape(Cn, HW)
        assert out.shape == (Cn, HW) and same_bits(out, np.ascontiguousarray(want))


@gpu
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("layout,Cn", LAYOUTS)
def test_pack_then_unpack_is_the_identity(layout, Cn, H, W):
    import wg_frame_store as FS
    stored, planar = frame_bytes(H, W, Cn, layout)
    floats = torch.from_numpy(stored.astype(np.float32) / 255.0).to(DEV)   # the frame's storage, in its own order
    packed, mismatches = FS.pack(floats)
    assert mismatches == 0 and packed.dtype == torch.uint8 and np.array_equal(packed.cpu().numpy(), stored)
    out = FS.unpack(packed, Cn, layout == "interleaved")
    assert same_bits(out.view(Cn, H, W), planar)


POISONS = {"half": np.float32(0.5), "minus_zero": np.float32(-0.0), "nan": np.uint32(0x7fc00abc).view(np.float32),
           "just_above_one": np.nextafter(np.float32(1), np.float32(2)), "minus_one_255th": np.float32(-1.0) / np.float32(255.0),
           "256_255ths": np.float32(256.0) / np.float32(255.0)}
# 33 x 17 x 3 = 1683 values: workgroups of 256, seven of them, and a tail of 3 behind the last whole group of four
PLACES = {"first_workgroup": 5, "middle_workgroup": 3 * 256 + 10, "last_workgroup": 6 * 256 + 21, "tail": 1682}


@gpu
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("poison", list(POISONS))
def test_pack_counts_exactly_the_poisoned_element_and_the_frame_is_served_from_float32(poison, place):
    import wg_frame_store as FS
    H, W = 33, 17
    stored, _ = frame_bytes(H, W, 3, "interleaved")
    storage = (stored.astype(np.float32) / 255.0)
    at = PLACES[place]
    storage[at] = POISONS[poison]
    assert storage.view(np.uint32)[at] == POISONS[poison].view(np.uint32)   # NumPy kept the bits (the NaN's payload, the zero's sign)
    packed, mismatches = FS.pack(torch.from_numpy(storage).to(DEV))
    want = stored.copy()
    want[at] = 0
    assert mismatches == 1 and np.array_equal(packed.cpu().numpy(), want)

    host = torch.from_numpy(np.moveaxis(storage.reshape(H, W, 3), -1, 0))   # as the reference lays an image out
    frames = FS.FrameList([host], DEV, 1 << 20)
    got = frames[0]
    assert frames.stats()["float32"] == 1 and frames.stats()["uint8"] == 0
    assert got.is_cuda and got.is_contiguous() and got.shape == host.shape and same_bits(got, host.to(DEV))
    assert bits(got).reshape(3, -1)[at % 3, at // 3] == POISONS[poison].view(np.uint32)
    got.zero_()
    assert same_bits(frames[0], host.to(DEV))


@gpu
def test_pack_counts_several_mismatches_across_workgroups():
    import wg_frame_store as FS
    n = 256 * 9 + 2
    storage = ((np.arange(n) % 256).astype(np.float32) / 255.0)
    where = [0, 255, 256, 1000, 2303, 2304, 2305]
    storage[where] = np.float32(0.3)
    _, mismatches = FS.pack(torch.from_numpy(storage).to(DEV))
    assert mismatches == len(where)


@gpu
def test_frame_lists_built_as_the_reference_builds_them(golden):
    import wg_frame_store as FS
    images, masks = host_lists()
    for name, t in zip(L.IMAGE_CASES + L.MASK_CASES, images + masks):
        assert same_bits(t, recorded(golden, name)) and strides(t) == strides(recorded(golden, name)), name
    budget = FS.Budget(1 << 20)
    for host, names in ((images, L.IMAGE_CASES), (masks, L.MASK_CASES)):
        frames = FS.FrameList(host, DEV, budget)
        assert len(frames) == len(host) and frames.stats()["pending"] == len(host)
        for i, name in enumerate(names):
            got = frames[i]
            again = frames[i]
            want = host[i].to(DEV)
            assert got.device == want.device and got.dtype == torch.float32 and got.shape == host[i].shape and got.is_contiguous(), name
            assert got.to(DEV) is got, name                            # the caller's `.to(device)` is a no-op
            assert same_bits(got, want), name
            assert got.data_ptr() != again.data_ptr(), name             # fresh storage per access
            got.fill_(7.0)
            assert same_bits(again, want) and same_bits(frames[i], want), name
        assert [same_bits(a, b.to(DEV)) for a, b in zip(frames, host)] == [True] * len(host)
        s = frames.stats()
        assert s["uint8"] == sum(n in L.EIGHT_BIT for n in names) and s["float32"] == len(names) - s["uint8"] and s["host_served"] == 0
        assert s["resident_bytes"] == sum(t.numel() * (1 if n in L.EIGHT_BIT else 4) for n, t in zip(names, host))
    assert budget.used == sum(t.numel() * (1 if n in L.EIGHT_BIT else 4) for n, t in zip(L.IMAGE_CASES + L.MASK_CASES, images + masks))


@gpu
def test_budget_that_admits_only_the_first_of_three_frames():
    import wg_frame_store as FS
    images, _ = host_lists()
    host = [images[0], images[1], images[0].clone()]
    frames = FS.FrameList(host, DEV, host[0].numel() * 4).prefetch()
    assert same_bits(frames[0], host[0].to(DEV)) and frames[0].is_cuda
    assert frames[1] is host[1] and frames[2] is host[2]
    s = frames.stats()
    assert (s["uint8"], s["float32"], s["host_served"], s["pending"]) == (1, 0, 2, 0)
    assert s["resident_bytes"] == host[0].numel() and s["budget_bytes"] == host[0].numel() * 4
    frames.release()
    assert frames[0] is host[0] and frames.budget.used == 0


@gpu
def test_unpack_on_a_non_default_stream():
    import wg_frame_store as FS
    images, _ = host_lists()
    frames = FS.FrameList([images[1]], DEV, 1 << 20).prefetch()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        got = frames[0]
        copy = got.clone()    # a read on that stream
    stream.synchronize()
    assert same_bits(copy, images[1].to(DEV)) and same_bits(got, images[1].to(DEV))


@gpu
def test_first_access_refuses_a_stream_capture_and_later_ones_capture():
    import wg_frame_store as FS
    images, _ = host_lists()
    frames = FS.FrameList([images[1], images[0]], DEV, 1 << 20)
    frames[0]   # adopted
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.stream(stream):
        graph.capture_begin()
        try:
            out = frames[0]
            try:
                frames[1]
            except RuntimeError as ex:
                refused = str(ex)
        finally:
            graph.capture_end()
    assert refused is not None and "stream capture" in refused
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, images[1].to(DEV))
    assert same_bits(frames[1], images[0].to(DEV))   # outside the capture the frame is adopted as usual


class CountingBackbone:
    """A stand-in for the DINO backbone: [1, 3, 14 h, 14 w] -> [1, 384, h, w], counting its calls."""
    num_heads = 6

    def __init__(self):
        self.calls = 0

    def get_intermediate_layers(self, x, n, reshape):
        assert n == [self.num_heads - 1] and reshape
        self.calls += 1
        h, w = x.shape[2] // 14, x.shape[3] // 14
        g = torch.Generator(device="cpu").manual_seed(h * 1000 + w)
        return [torch.randn(1, 384, h, w, generator=g).to(x.device) * x.flatten()[0]]


class UncertaintyStub:
    """The two members of the reference's UncertaintyModel the store touches (method.py:255-265, restated)."""

    def __init__(self):
        self.backbone = CountingBackbone()
        self._images_cache = {}

    def _get_dino_cached(self, x, cache_entry=None):
        if cache_entry is None or (cache_entry, x.shape) not in self._images_cache:
            with torch.no_grad():
                x = self.backbone.get_intermediate_layers(x, n=[self.backbone.num_heads - 1], reshape=True)[-1]
            if cache_entry is not None:
                self._images_cache[(cache_entry, x.shape)] = x.detach().cpu()
        else:
            x = self._images_cache[(cache_entry, x.shape)].to(x.device)
        return x


@gpu
def test_feature_cache_through_the_callers_get_dino_cached():
    """As in the reference, the key's shape is that of the backbone's OUTPUT, so a second call with the same input looks up the input's
    shape: the stub is called with feature-shaped inputs the second time, exactly as the reference's method would be."""
    import wg_frame_store as FS
    model = UncertaintyStub()
    model._images_cache = FS.FeatureCache(DEV, 1 << 24)
    small, large = torch.full((1, 3, 42, 28), 1.5, device=DEV), torch.full((1, 3, 350, 350), 0.5, device=DEV)
    first = {}
    for name, x in (("small", small), ("large", large)):
        first[name] = model._get_dino_cached(x, cache_entry=7)
    assert model.backbone.calls == 2 and first["small"].shape == (1, 384, 3, 2) and first["large"].shape == (1, 384, 25, 25)
    assert set(model._images_cache) == {(7, first["small"].shape), (7, first["large"].shape)} and len(model._images_cache) == 2
    assert model._images_cache.stats()["resident"] == 0   # nothing is uploaded before it is read
    for name in ("small", "large"):
        probe = torch.empty(first[name].shape, device=DEV)   # an input whose shape is the key's
        again = model._get_dino_cached(probe, cache_entry=7)
        assert again.is_cuda and again.to(DEV) is again and same_bits(again, first[name])
        assert again is model._images_cache[(7, first[name].shape)]
    assert model.backbone.calls == 2
    s = model._images_cache.stats()
    assert s["resident"] == 2 and s["resident_bytes"] == 4 * 384 * (6 + 625) and s["host_served"] == 0
    host = model._images_cache.to_host_dict()
    assert type(host) is dict and all(not v.is_cuda and same_bits(v, model._images_cache[k]) for k, v in host.items())
    del model._images_cache[(7, first["small"].shape)]
    assert model._images_cache.stats()["resident_bytes"] == 4 * 384 * 625 and (7, first["small"].shape) not in model._images_cache


@gpu
def test_opt_in_on_a_stand_in_trainer_and_undo():
    import wg_integration
    from wg_frame_store import FeatureCache, FrameList
    images, masks = host_lists()
    masks = [masks[0], masks[1], masks[0].clone(), masks[1].clone()][:len(images)]
    um = UncertaintyStub()
    before = torch.full((1, 3, 28, 28), 2.0, device=DEV)
    kept = um._get_dino_cached(before, cache_entry=0)       # an entry cached BEFORE the switch
    trainer = types.SimpleNamespace(train_images=images, train_masks=masks, model=types.SimpleNamespace(uncertainty_model=um))
    plain = [(images[i].to(DEV), masks[i].to(DEV)) for i in range(len(images))]

    undo = wg_integration.keep_training_frames_on_device(trainer, device=DEV, max_device_bytes=1 << 24)
    assert isinstance(trainer.train_images, FrameList) and isinstance(trainer.train_masks, FrameList) and isinstance(um._images_cache, FeatureCache)
    for camera_id in range(len(images)):   # one step's worth of accesses per frame, in the caller's words
        gt_image = trainer.train_images[camera_id].to(DEV)
        mask = trainer.train_masks[camera_id].to(DEV) if trainer.train_masks is not None else None
        assert same_bits(gt_image, plain[camera_id][0]) and same_bits(mask, plain[camera_id][1])
        assert gt_image.shape == images[camera_id].shape and mask.shape == masks[camera_id].shape
    x = torch.full((1, 3, 42, 28), 1.5, device=DEV)
    new = um._get_dino_cached(x, cache_entry=1)             # an entry cached WHILE the switch is on
    assert same_bits(um._get_dino_cached(torch.empty(new.shape, device=DEV), cache_entry=1), new)
    old_again = um._get_dino_cached(torch.empty(kept.shape, device=DEV), cache_entry=0)
    assert same_bits(old_again, kept) and old_again.is_cuda and um.backbone.calls == 2
    st = undo.stats()
    assert st["images"]["uint8"] == 2 and st["images"]["float32"] == 2 and st["masks"]["uint8"] == 4 and st["features"]["resident"] == 2
    assert 0 < st["used_bytes"] <= st["budget_bytes"] == 1 << 24
    keys = set(um._images_cache)

    undo()
    assert trainer.train_images is images and trainer.train_masks is masks
    assert type(um._images_cache) is dict and set(um._images_cache) == keys == {(0, kept.shape), (1, new.shape)}
    assert all(not v.is_cuda for v in um._images_cache.values())
    assert same_bits(um._images_cache[(0, kept.shape)], kept) and same_bits(um._images_cache[(1, new.shape)], new)
    assert same_bits(trainer.train_images[0].to(DEV), plain[0][0])
