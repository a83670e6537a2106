#!/usr/bin/env python3
"""What one training step's input fetches cost: the caller's `host.to(device)` against wg_frame_store, on the same GPU in the same run.

    python scripts/bench_frame_store.py [--calls 30] [--warmup 5] [--out profiles/frame_store/bench.json]

Per size (1600x1200, 1920x1080) eight distinct frames are built exactly as wildgaussians/method.py:1716-1723 builds them (a float32
[3, H, W] view of H x W x 3 storage, a float32 [1, H, W] mask, pageable host memory) with the two backbone-feature entries of a frame
([1, 384, H/14, W/14] and the 350-pixel grid).  Legs, alternating call by call and cycling over the eight frames so that no leg re-reads a
warm staging buffer:

    parent_all      image + mask + the two feature entries, each `host.to(device)`           (the yardstick)
    store_all       the same four fetches through FrameList / FeatureCache, each followed by the caller's `.to(device)`
    parent_frames   image + mask only
    store_frames    image + mask only through FrameList

Host wall time around each call, ended by a device synchronise (the parent's copy blocks the host).  Medians with p10 / p90.  Also: the
one-off adoption cost per frame (first access of image + mask: upload, pack, one word read back) and the resident bytes per frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wild-gaussians_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAMES = 8


def convert_image_dtype(image, dtype):   # the uint8 -> float32 branch of the caller's function
    return image.astype(dtype) / 255.0


def make_frames(H, W, seed):
    import wg_fused_uncertainty as U
    rng = np.random.default_rng(seed)
    g = U.Geometry(H, W, 14)
    images, masks, feats = [], [], []
    for _ in range(FRAMES):
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        msk = (rng.integers(0, 4, size=(H, W), dtype=np.uint8) > 0).astype(np.uint8) * 255
        images.append(torch.from_numpy(np.moveaxis(convert_image_dtype(img, np.float32), -1, 0)))
        masks.append(torch.from_numpy(convert_image_dtype(msk, np.float32)[None]))
        feats.append((torch.from_numpy(rng.standard_normal((1, 384, g.hp, g.wp), dtype=np.float32)),
                      torch.from_numpy(rng.standard_normal((1, 384, g.hd, g.wd), dtype=np.float32))))
    return images, masks, feats


def summary(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4), "calls": len(ms)}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) * 1e3
    del out
    return dt


def run_size(H, W, dev, calls, warmup):
    import wg_frame_store as FS
    images, masks, feats = make_frames(H, W, seed=H)
    budget = FS.Budget(None, dev)
    f_images, f_masks = FS.FrameList(images, dev, budget), FS.FrameList(masks, dev, budget)
    cache = FS.FeatureCache(dev, budget)
    for i, (a, b) in enumerate(feats):
        cache[(i, a.shape)] = a
        cache[(i, b.shape)] = b
    FS.FrameList([images[0][:, :8, :8].contiguous()], dev, 1 << 20)[0]   # code objects loaded before anything is timed
    adoption = [timed(lambda i=i: (f_images[i], f_masks[i]), dev) for i in range(FRAMES)]
    feature_upload = [timed(lambda i=i: (cache[(i, feats[i][0].shape)], cache[(i, feats[i][1].shape)]), dev) for i in range(FRAMES)]

    legs = {
        "parent_all": lambda i: (images[i].to(dev), masks[i].to(dev), feats[i][0].to(dev), feats[i][1].to(dev)),
        "store_all": lambda i: (f_images[i].to(dev), f_masks[i].to(dev), cache[(i, feats[i][0].shape)].to(dev), cache[(i, feats[i][1].shape)].to(dev)),
        "parent_frames": lambda i: (images[i].to(dev), masks[i].to(dev)),
        "store_frames": lambda i: (f_images[i].to(dev), f_masks[i].to(dev)),
    }
    times = {k: [] for k in legs}
    for n in range(warmup + calls):
        for name, fn in legs.items():
            dt = timed(lambda: fn(n % FRAMES), dev)
            if n >= warmup:
                times[name].append(dt)
    # the store delivers the parent's bits: checked on the frames that were timed
    for i in range(FRAMES):
        assert torch.equal(f_images[i].view(torch.int32), images[i].to(dev).contiguous().view(torch.int32))
        assert torch.equal(f_masks[i].view(torch.int32), masks[i].to(dev).view(torch.int32))
    host_bytes = {"image": images[0].numel() * 4, "mask": masks[0].numel() * 4, "features": sum(t.numel() * 4 for t in feats[0])}
    out = {"size": [W, H], "frames": FRAMES, "host_bytes_per_frame": host_bytes, "legs": {k: summary(v) for k, v in times.items()},
           "adoption_ms_per_frame_image_and_mask": summary(adoption), "feature_first_read_ms_per_frame": summary(feature_upload),
           "resident_bytes_per_frame": {"image": f_images.stats()["resident_bytes"] // FRAMES, "mask": f_masks.stats()["resident_bytes"] // FRAMES,
                                        "features": cache.stats()["resident_bytes"] // FRAMES},
           "stats": {"images": f_images.stats(), "masks": f_masks.stats(), "features": cache.stats()}}
    L = out["legs"]
    out["parent_over_store_all"] = round(L["parent_all"]["median_ms"] / L["store_all"]["median_ms"], 2)
    out["parent_over_store_frames"] = round(L["parent_frames"]["median_ms"] / L["store_frames"]["median_ms"], 2)
    out["adoption_over_parent_frames_fetch"] = round(out["adoption_ms_per_frame_image_and_mask"]["median_ms"] / L["parent_frames"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1600x1200,1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_store", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_store.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = {"what": "host wall time per call ended by a device synchronise; legs alternate call by call over 8 distinct frames",
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "sizes": []}
    for s in args.sizes.split(","):
        W, H = (int(v) for v in s.split("x"))
        result["sizes"].append(run_size(H, W, dev, args.calls, args.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "sizes": [{k: s[k] for k in ("size", "parent_over_store_all", "parent_over_store_frames",
                                                                    "adoption_over_parent_frames_fetch")} for s in result["sizes"]]}))


if __name__ == "__main__":
    main()
