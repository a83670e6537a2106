"""Per-Gaussian contribution statistics of rendered frames (beyond the reference): the caller-owned arrays the contribution pass
(wg_render_contributions, csrc/contrib/contrib.hip) combines into, the context manager that feeds them from a caller that cannot pass
keywords, and the argument checks of ``GaussianRasterizer.forward(..., contributions=, contribution_mask=)``.  Pure torch: no native call
is made here."""
import contextlib
import threading

import torch

Q32 = 4294967296.0   # 2^32: weight_sum_q32 holds the sum of floor(w * 2^32)

STATS_MSG = "contributions must be a ContributionStats whose three tensors hold P elements on the call's HIP device"
MASK_MSG = "contribution_mask must be a bool or float32 tensor of shape [H, W] or [1, H, W] (or H * W elements) on the call's HIP device"


class ContributionStats:
    """What each of P Gaussians contributed to the frames swept so far, over the (pixel, Gaussian) pairs the forward calls blended, with
    w = alpha * T the blend weight:

    * ``max_weight``      float32 [P]: the largest w;
    * ``hits``            int64 [P]: the number of pairs;
    * ``weight_sum_q32``  int64 [P]: the sum of floor(w * 2^32) -- fixed point, so that the sum is an integer one and two sweeps give the
      same bits whatever order the tiles ran in; ``weight_sum`` is the float64 view of it;
    * ``views``           how many frames were combined (a Python int).

    Pass it as ``GaussianRasterizer.forward(..., contributions=stats)`` or through ``with collect_contributions(stats): ...``."""

    def __init__(self, P: int, device="cuda"):
        P = int(P)
        if P < 0:
            raise ValueError("P must not be negative")
        self.max_weight = torch.zeros(P, dtype=torch.float32, device=device)
        self.hits = torch.zeros(P, dtype=torch.int64, device=device)
        self.weight_sum_q32 = torch.zeros(P, dtype=torch.int64, device=device)
        self.views = 0

    @property
    def P(self) -> int:
        return self.hits.numel()

    @property
    def device(self) -> torch.device:
        return self.hits.device

    @property
    def weight_sum(self) -> torch.Tensor:
        """float64 [P]: weight_sum_q32 * 2^-32 (an exact conversion while a Gaussian's summed weight stays below 2^21)."""
        return self.weight_sum_q32.to(torch.float64) * (1.0 / Q32)

    def reset(self) -> "ContributionStats":
        self.max_weight.zero_()
        self.hits.zero_()
        self.weight_sum_q32.zero_()
        self.views = 0
        return self

    def merge_(self, other: "ContributionStats") -> "ContributionStats":
        """Combine another sweep's statistics into this one (max / add / add; views add): for ranks that swept different views."""
        if not isinstance(other, ContributionStats) or other.P != self.P:
            raise ValueError("merge_ needs a ContributionStats of the same P")
        dev = self.device
        # (torch.maximum propagates NaN, as the unsigned-integer maximum of the bit patterns does)
        torch.maximum(self.max_weight, other.max_weight.to(dev), out=self.max_weight)
        self.hits += other.hits.to(dev)
        self.weight_sum_q32 += other.weight_sum_q32.to(dev)
        self.views += other.views
        return self

    def keep_mask(self, min_max_weight=None, min_hits=None, min_weight_sum=None) -> torch.Tensor:
        """bool [P]: the Gaussians that meet EVERY given threshold (max_weight >= min_max_weight, hits >= min_hits, weight_sum >=
        min_weight_sum); a threshold left None does not take part, none given keeps everything.  A NaN max_weight is kept."""
        keep = torch.ones(self.P, dtype=torch.bool, device=self.device)
        if min_max_weight is not None:
            keep &= ~(self.max_weight < float(min_max_weight))
        if min_hits is not None:
            keep &= self.hits >= int(min_hits)
        if min_weight_sum is not None:
            keep &= self.weight_sum >= float(min_weight_sum)
        return keep

    def __repr__(self):
        return f"ContributionStats(P={self.P}, device={self.device}, views={self.views})"


def check_stats(stats, P: int, device) -> None:
    """What `contributions=` may be: raises before anything is rendered."""
    if not isinstance(stats, ContributionStats):
        raise Exception(STATS_MSG)
    for t, dtype in ((stats.max_weight, torch.float32), (stats.hits, torch.int64), (stats.weight_sum_q32, torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or t.numel() != int(P) or not t.is_contiguous() or t.device != device:
            raise Exception(STATS_MSG)


def check_mask(mask, H: int, W: int, device):
    """What `contribution_mask=` may be -> the float32 tensor of H * W elements the native call reads (a bool mask converted; 0 = the pixel
    takes no part), or None.  Raises before anything is rendered."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.float32) or mask.device != device:
        raise Exception(MASK_MSG)
    if tuple(mask.shape) not in ((H, W), (1, H, W), (H * W,)):
        raise Exception(MASK_MSG)
    return mask.detach().to(torch.float32).reshape(H * W).contiguous()


# ---- the calling thread's default: `with collect_contributions(stats, mask): ...` for callers that cannot pass keywords.  It feeds the FIRST
# forward call of the block only: a caller's render makes two or three rasterizer calls over the same geometry (the image, a depth render,
# ...), and feeding each would count every pair two or three times.
_tls = threading.local()


@contextlib.contextmanager
def collect_contributions(stats, mask=None):
    if not isinstance(stats, ContributionStats):
        raise Exception(STATS_MSG)
    saved = getattr(_tls, "pending", None)
    _tls.pending = [stats, mask]
    try:
        yield stats
    finally:
        _tls.pending = saved


def take_pending():
    """(stats, mask) of the innermost open `collect_contributions` block if no forward call of it has taken them yet (and marks them taken),
    else (None, None)."""
    pending = getattr(_tls, "pending", None)
    if pending is None or pending[0] is None:
        return None, None
    stats, mask = pending
    pending[0] = None
    return stats, mask


def restore_pending(stats, mask) -> None:
    """Give back what take_pending() handed out: the call that took it was refused before it rendered anything."""
    pending = getattr(_tls, "pending", None)
    if pending is not None and pending[0] is None:
        pending[0], pending[1] = stats, mask
