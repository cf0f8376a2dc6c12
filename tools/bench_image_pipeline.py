#!/usr/bin/env python3
"""Time the image-folder pipeline's hot path on the GPU.

Builds a seeded synthetic store (default 4,096 random images of about
256x341, ~1 GB: past the 256 MiB Infinity Cache, so the reads come from
HBM) and times, at B=256, S=224, bf16:

  (a) loader  one full GPUImageLoader step: box sampling + meta upload +
              the fused kernel
  (b) kernel  the fused kernel alone, geometry already on the device
  (c) eager   what a user would write without it, on the same GPU:
              per-sample slice -> F.interpolate(antialias=True) ->
              window / flip / normalise -> stack -> channels_last

Device events around windows of at least --window seconds, after a warm-up,
the three variants alternating over --rounds rounds; the median round is
reported. The kernel's bytes/s comes from shapes: box bytes read plus
output bytes written. Prints one JSON line. There is no CPU fallback: a
time is a GPU time or it is not reported.
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from noisynet_amd import image_pipeline as ip  # noqa: E402
from noisynet_amd import ops  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X HBM3E spec


def synthetic_store(n, seed, device, store_device):
    rng = np.random.default_rng(seed)
    H = np.full(n, 256, dtype=np.int64)
    W = rng.integers(300, 384, n)            # mean 341
    swap = rng.random(n) < 0.25              # a quarter portrait
    H, W = np.where(swap, W, H), np.where(swap, H, W)
    nbytes = 3 * H * W
    offsets = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
    arena = rng.integers(0, 256, int(nbytes.sum()), dtype=np.uint8)
    index = np.stack([offsets, H, W, rng.integers(0, 1000, n)], 1)
    return ip.ImageStore.from_arrays(arena, index.astype(np.int64),
                                     [str(i) for i in range(1000)],
                                     device=device, store_device=store_device)


def train_meta(store, idx, S, rng):
    H, W = store.H[idx], store.W[idx]
    meta = np.zeros((len(idx), 11), dtype=np.int32)
    meta[:, 0], meta[:, 1] = H, W
    meta[:, 2], meta[:, 3], meta[:, 4], meta[:, 5] = \
        ip.random_resized_boxes(H, W, rng)
    meta[:, 6] = S
    meta[:, 7] = S
    meta[:, 10] = rng.integers(0, 2, len(idx))
    return meta


def eager_batch(arena, offsets, meta, S, dtype):
    """Composition of stock torch ops on the GPU (zero mean, unit std)."""
    out = []
    for off, m in zip(offsets.tolist(), meta.tolist()):
        H, W, x0, y0, bw, bh, oh, ow, oy, ox, flip = m
        img = arena[off:off + 3 * H * W].view(H, W, 3)
        box = img[y0:y0 + bh, x0:x0 + bw].permute(2, 0, 1).float() / 255.0
        r = F.interpolate(box[None], size=(oh, ow), mode='bilinear',
                          antialias=True, align_corners=False)[0]
        r = r[:, oy:oy + S, ox:ox + S]
        out.append(r.flip(-1) if flip else r)
    return torch.stack(out).to(dtype).contiguous(
        memory_format=torch.channels_last)


def timed(fn, window, min_calls=3):
    """images-independent: seconds per call over a window >= ``window``."""
    calls, total = 0, 0.0
    while total < window or calls < min_calls:
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        n = fn()
        stop.record()
        stop.synchronize()
        total += start.elapsed_time(stop) / 1e3
        calls += n
    return total / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--store_device', default='cuda',
                    choices=['cuda', 'host'])
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_pipeline needs a GPU: nothing measured')
    device = torch.device('cuda')
    dtype = torch.bfloat16
    B, S = args.batch, args.size

    store = synthetic_store(args.images, args.seed, device, args.store_device)
    loader = ip.GPUImageLoader(store, B, size=S, train=True, dtype=dtype,
                               seed=args.seed)

    # fixed batch for (b) and (c), geometry resident on the device
    rng = np.random.default_rng(args.seed + 1)
    idx = rng.permutation(len(store))[:B]
    meta = train_meta(store, idx, S, rng)
    offsets = np.ascontiguousarray(store.offsets[idx])
    arena = store.arena if store.arena.is_cuda else store.arena.to(device)
    off_d, meta_d = ops.functional.upload_crop_request(offsets, meta, device)
    ops.crop_resize_mirror_normalize(arena, off_d, meta_d, S, out_dtype=dtype,
                                     host_copies=(offsets, meta))  # validates
    ext = ops.ext()
    zero, one = [0.0] * 3, [1.0] * 3
    kernel_reps = 20

    def run_loader():
        n = 0
        for _ in loader:
            n += 1
        loader.set_epoch(loader.epoch + 1)
        return n

    def run_kernel():
        for _ in range(kernel_reps):
            ext.crop_resize_mirror_normalize(arena, off_d, meta_d, S, zero,
                                             one, 1)
        return kernel_reps

    def run_eager():
        eager_batch(arena, offsets, meta, S, dtype)
        return 1

    variants = {'loader': run_loader, 'kernel': run_kernel,
                'eager': run_eager}

    # results must agree before speeds are compared
    fused = ext.crop_resize_mirror_normalize(arena, off_d, meta_d, S, zero,
                                             one, 1).float()
    diff = (fused - eager_batch(arena, offsets, meta, S, dtype).float())
    max_diff = float(diff.abs().max())

    for fn in variants.values():        # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):        # alternate the variants
        for name, fn in variants.items():
            rounds[name].append(timed(fn, args.window))
    sec = {k: statistics.median(v) for k, v in rounds.items()}

    box_bytes = int((3 * meta[:, 4].astype(np.int64) * meta[:, 5]).sum())
    out_bytes = B * 3 * S * S * 2
    bytes_per_s = (box_bytes + out_bytes) / sec['kernel']
    print(json.dumps({
        'bench': 'image_pipeline', 'device': torch.cuda.get_device_name(0),
        'images': args.images, 'arena_mb': round(store.nbytes / 1e6, 1),
        'store_device': store.store_device, 'batch': B, 'size': S,
        'dtype': 'bf16', 'window_s': args.window, 'rounds': args.rounds,
        'loader_step_ms': round(sec['loader'] * 1e3, 4),
        'kernel_ms': round(sec['kernel'] * 1e3, 4),
        'eager_ms': round(sec['eager'] * 1e3, 4),
        'loader_img_per_s': round(B / sec['loader'], 1),
        'kernel_img_per_s': round(B / sec['kernel'], 1),
        'eager_img_per_s': round(B / sec['eager'], 1),
        'rounds_ms': {k: [round(t * 1e3, 4) for t in v]
                      for k, v in rounds.items()},
        'kernel_box_bytes_read': box_bytes,
        'kernel_out_bytes_written': out_bytes,
        'kernel_gb_per_s': round(bytes_per_s / 1e9, 1),
        'kernel_share_of_hbm_peak': round(bytes_per_s / HBM_PEAK_BYTES_PER_S,
                                          4),
        'fused_vs_eager_max_abs_diff_bf16': max_diff,
    }))


if __name__ == '__main__':
    main()
