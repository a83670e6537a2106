"""Device-resident training frames -- an opt-in store for what `WildGaussians.train_iteration` fetches from the host on every step
(wildgaussians/method.py:1917-1918 and :264): the ground-truth image, its mask and the cached backbone features
(include/wg_frames.h, csrc/frames/frames.hip).

    from wg_frame_store import FrameList, FeatureCache, Budget
    budget = Budget(max_device_bytes)                       # None: half of the device memory that is free now
    trainer.train_images = FrameList(trainer.train_images, device, budget)
    gt = trainer.train_images[i].to(device)                 # the caller's line, unchanged: `.to` is now a no-op

`FrameList` stands in for `train_images` / `train_masks`.  The reference builds these float32 tensors from 8-bit files as
`astype(np.float32) / 255.0`, so every value is exactly k / 255 and a frame is one byte per value of information.  At its first access a
frame is uploaded once (its dense storage, in its own memory order: the image's is H x W x 3), `wg_frames_pack` turns it into uint8 and
counts the values that are NOT exactly k / 255, and one word is read back.  Zero: the uint8 copy is kept, and every access runs
`wg_frames_unpack` into a fresh planar float32 tensor whose bits are those of `host.to(device)`.  Anything else (a float dataset, a 16-bit
source, NaN, -0.0): the float32 device copy is kept and every access returns a clone of it.  The contract is shape, dtype and values, not
strides: the result is contiguous.

`FeatureCache` stands in for `UncertaintyModel._images_cache`: a dict whose values move to the device when they are first read, unchanged
(no quantisation).

What is not covered keeps the reference's behaviour -- the host tensor goes out and the caller's `.to` copies it: a tensor that is not float32,
not 3-dimensional with 1..4 channels in front, neither contiguous nor pixel-major, and whatever `plan_residency` does not admit to the budget.
"""
from __future__ import annotations

import ctypes as C

import torch

from diff_gaussian_rasterization import _C as _native

_lib = _native._lib
_lib.wg_frames_pack_scratch_words.restype = C.c_size_t
_lib.wg_frames_pack_scratch_words.argtypes = [C.c_size_t]
_lib.wg_frames_pack.restype = C.c_int
_lib.wg_frames_pack.argtypes = [C.c_size_t] + [C.c_void_p] * 4
_lib.wg_frames_unpack.restype = C.c_int
_lib.wg_frames_unpack.argtypes = [C.c_int, C.c_size_t, C.c_int] + [C.c_void_p] * 3

MAX_CHANNELS = 4


# ---------------------------------------------------------------------------------------------- residency
def plan_residency(nbytes, budget) -> list:
    """Which entries live on the device: entries are walked in index order and one is admitted while the running total stays within
    `budget` bytes.  An entry that does not fit is refused; later, smaller ones may still be admitted."""
    plan, total = [], 0
    for n in nbytes:
        n = int(n)
        fits = total + n <= budget
        plan.append(fits)
        if fits:
            total += n
    return plan


class Budget:
    """Device bytes the store may hold: `total`, of which `used` are taken.  One object is shared by the lists and the cache of one trainer."""

    def __init__(self, total=None, device=None):
        if total is None:   # half of what is free now
            total = torch.cuda.mem_get_info(device)[0] // 2
        self.total, self.used = int(total), 0

    @property
    def free(self) -> int:
        return max(self.total - self.used, 0)

    def take(self, n: int) -> bool:
        if self.used + n > self.total:
            return False
        self.used += n
        return True

    def give_back(self, n: int) -> None:
        self.used -= n


def _as_budget(budget, device) -> Budget:
    return budget if isinstance(budget, Budget) else Budget(budget, device)


# ---------------------------------------------------------------------------------------------- tensor-level pieces
def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def pack(src: torch.Tensor):
    """float32 device tensor (contiguous) -> (uint8 tensor of the same shape, the number of values that are not exactly k / 255).
    Reads one word back: not inside a stream capture."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.numel() > 0):
        raise RuntimeError("wg_frame_store.pack: a non-empty contiguous float32 tensor on a HIP device is required (there is no CPU path)")
    dev, n = src.device, src.numel()
    with torch.cuda.device(dev):
        dst = torch.empty(src.shape, device=dev, dtype=torch.uint8)
        partials = torch.empty(_lib.wg_frames_pack_scratch_words(n), device=dev, dtype=torch.int32)
        _native._check(_lib.wg_frames_pack(n, src.data_ptr(), dst.data_ptr(), partials.data_ptr(), _stream(dev)), "wg_frames_pack")
        mismatches = int(partials[0].item()) & 0xffffffff
    return dst, mismatches


def unpack(src: torch.Tensor, channels: int, interleaved: bool, out: torch.Tensor = None) -> torch.Tensor:
    """uint8 device tensor of channels * HW bytes (pixel-major when `interleaved`, planar otherwise) -> float32 [channels, HW], each value
    (float)byte / 255.0f.  `out`: a contiguous float32 tensor of channels * HW elements to write into."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()):
        raise RuntimeError("wg_frame_store.unpack: a contiguous uint8 tensor on a HIP device is required (there is no CPU path)")
    channels = int(channels)
    if not 1 <= channels <= MAX_CHANNELS or src.numel() == 0 or src.numel() % channels:
        raise RuntimeError("wg_frame_store.unpack: 1..4 channels and a whole number of pixels are expected")
    dev, HW = src.device, src.numel() // channels
    if out is None:
        out = torch.empty((channels, HW), device=dev, dtype=torch.float32)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == src.numel()):
        raise RuntimeError("wg_frame_store.unpack: `out` must be a contiguous float32 tensor of channels * HW elements on the same device")
    with torch.cuda.device(dev):
        _native._check(_lib.wg_frames_unpack(channels, HW, int(bool(interleaved)), src.data_ptr(), out.data_ptr(), _stream(dev)),
                       "wg_frames_unpack")
    return out


# ---------------------------------------------------------------------------------------------- FrameList
def _layout(t):
    """"planar" / "interleaved" for a frame the store covers, None otherwise."""
    if not (torch.is_tensor(t) and not t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.numel() > 0
            and 1 <= t.shape[0] <= MAX_CHANNELS and not t.requires_grad):
        return None
    if t.is_contiguous():
        return "planar"
    if t.permute(1, 2, 0).is_contiguous():   # H x W x C storage: np.moveaxis(image, -1, 0)
        return "interleaved"
    return None


class _Frame:
    __slots__ = ("kind", "data", "interleaved", "reserved")   # kind: "uint8" / "float32"


class FrameList:
    """A read-only sequence over `host_tensors`: `frames[i]` is a FRESH contiguous float32 tensor on `device` with the shape of
    `host_tensors[i]` and the bits of `host_tensors[i].to(device)` -- or `host_tensors[i]` itself for a frame the store does not hold.
    `budget`: bytes, a `Budget`, or None for half of the free device memory.  Residency is planned at construction (`plan_residency`) with
    4 bytes per value; a frame that turns out to be 8-bit hands 3 of the 4 back to the budget when it is adopted."""

    def __init__(self, host_tensors, device, budget=None):
        self.host = host_tensors   # the caller's own list: kept, never modified, never freed
        self.device = torch.device(device)
        self._layouts = [_layout(t) for t in host_tensors]
        wanted = [i for i, l in enumerate(self._layouts) if l is not None]
        self.budget = _as_budget(budget, self.device) if wanted or budget is not None else None
        plan = plan_residency([host_tensors[i].numel() * 4 for i in wanted], self.budget.free) if wanted else []
        self._resident = [False] * len(host_tensors)
        for i, ok in zip(wanted, plan):
            self._resident[i] = ok
            if ok:
                self.budget.take(host_tensors[i].numel() * 4)
        self._frames = [None] * len(host_tensors)

    def __len__(self):
        return len(self.host)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def _adopt(self, i):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("wg_frame_store: the first access of a frame reads one word back from the device and cannot run inside a stream "
                               "capture; call prefetch() before capturing")
        t, f = self.host[i], _Frame()
        f.interleaved = self._layouts[i] == "interleaved"
        flat = (t.permute(1, 2, 0) if f.interleaved else t).reshape(-1)   # a view: the storage as it lies
        with torch.cuda.device(self.device):
            dev = flat.to(self.device)
            packed, mismatches = pack(dev)
            f.reserved = t.numel() * 4
            if mismatches == 0:
                f.kind, f.data = "uint8", packed
                self.budget.give_back(t.numel() * 3)
                f.reserved = t.numel()
            else:   # kept planar, so that an access is one clone
                f.kind = "float32"
                f.data = dev.view(t.shape[1], t.shape[2], t.shape[0]).permute(2, 0, 1).contiguous() if f.interleaved else dev.view(t.shape)
        self._frames[i] = f
        return f

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        i = range(len(self))[i]   # negative indices, IndexError
        if not self._resident[i]:
            return self.host[i]
        f = self._frames[i] or self._adopt(i)
        if f.kind == "float32":
            return f.data.clone()
        shape = self.host[i].shape
        with torch.cuda.device(self.device):
            out = torch.empty(shape, device=self.device, dtype=torch.float32)
        return unpack(f.data, shape[0], f.interleaved, out=out)

    def prefetch(self):
        """Adopt every resident frame now (one upload, one pack and one host read each)."""
        for i in range(len(self)):
            if self._resident[i] and self._frames[i] is None:
                self._adopt(i)
        return self

    def stats(self) -> dict:
        frames = [f for f in self._frames if f is not None]
        return {"frames": len(self), "uint8": sum(f.kind == "uint8" for f in frames), "float32": sum(f.kind == "float32" for f in frames),
                "pending": sum(r and f is None for r, f in zip(self._resident, self._frames)),
                "host_served": sum(not r for r in self._resident),
                "resident_bytes": sum(f.data.numel() * f.data.element_size() for f in frames),
                "budget_bytes": self.budget.total if self.budget is not None else 0}

    def release(self):
        """Drop the device copies and hand their bytes back to the budget; every frame is served from the host afterwards."""
        for i, f in enumerate(self._frames):
            if f is not None:
                self.budget.give_back(f.reserved)
            elif self._resident[i]:
                self.budget.give_back(self.host[i].numel() * 4)
        self._frames = [None] * len(self.host)
        self._resident = [False] * len(self.host)


# ---------------------------------------------------------------------------------------------- FeatureCache
class FeatureCache(dict):
    """`UncertaintyModel._images_cache` with its values on the device.  `cache[key] = x.detach().cpu()` (method.py:262) keeps the tensor it is
    given; the FIRST `cache[key]` moves it to the device while the budget admits it, and from then on `cache[key]` returns that device tensor,
    so the caller's `.to(device)` (method.py:264) is a no-op.  An entry that is never read costs nothing: the reference's own
    `_get_dino_cached` stores under the shape of the backbone's OUTPUT and looks up under the shape of its INPUT, so on the unchanged reference
    no look-up ever hits and only a caller whose two keys agree reads this cache at all.  Values are stored unchanged (no quantisation); what
    is not a float32 CPU tensor, and what the budget does not admit, is kept and returned as it came.  `in`, `len`, `del`, iteration: a
    dict's."""

    def __init__(self, device, budget=None, initial=None):
        super().__init__()
        self.device = torch.device(device)
        self.budget = _as_budget(budget, self.device)
        self._taken = {}   # key -> bytes taken from the budget: the entries that live on the device
        for k, v in (initial or {}).items():
            self[k] = v

    def _forget(self, key):
        n = self._taken.pop(key, 0)
        if n:
            self.budget.give_back(n)

    def __setitem__(self, key, value):
        self._forget(key)
        super().__setitem__(key, value)

    def __getitem__(self, key):
        value = super().__getitem__(key)
        if torch.is_tensor(value) and not value.is_cuda and value.dtype == torch.float32 and value.numel() > 0:
            n = value.numel() * value.element_size()
            if self.budget.take(n):
                self._taken[key] = n
                value = value.detach().to(self.device)
                super().__setitem__(key, value)
        return value

    def __delitem__(self, key):
        super().__delitem__(key)
        self._forget(key)

    def pop(self, key, *default):
        value = super().pop(key, *default)
        self._forget(key)
        return value

    def popitem(self):
        key, value = super().popitem()
        self._forget(key)
        return key, value

    def clear(self):
        super().clear()
        for key in list(self._taken):
            self._forget(key)

    def update(self, *args, **kwargs):
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    def setdefault(self, key, default=None):
        if key not in self:
            self[key] = default
        return self[key]

    def to_host_dict(self) -> dict:
        """A plain dict with a CPU copy of every entry: what the reference's own cache would hold."""
        return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.items()}

    def stats(self) -> dict:
        return {"entries": len(self), "resident": len(self._taken), "host_served": len(self) - len(self._taken),
                "resident_bytes": sum(self._taken.values()), "budget_bytes": self.budget.total}
