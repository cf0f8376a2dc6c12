"""Image-folder ingestion for the ImageNet driver.

Same design as the CIFAR path (``data.py``): decode the dataset once, keep
it resident as packed ``uint8``, and do all per-step augmentation on the GPU
inside the loop. Images differ in size here, so they live back to back in
one byte arena with an index (offset, H, W, label) and one HIP kernel
(``ops.crop_resize_mirror_normalize``) does crop, antialiased resize, mirror,
normalise, cast and NHWC layout for a whole batch per step. This replaces
the reference's DALI pipelines (utils.py:63-116: fused decode + random crop,
triangular Resize, CropMirrorNormalize).

  ImageStore            scan + decode (PIL, thread pool) + pack + cache
  random_resized_boxes  vectorised random-resized-crop sampler (DALI ranges)
  center_boxes          "resize shorter side, centre crop" geometry
  GPUImageLoader        iterable of (images, target) for train()/validate()
"""

import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from .timm.data.dataset import find_images_and_targets

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_CACHE_VERSION = 1
_MAX_WORKERS = 16


def _round(x):
    """Round half up, as integers (numpy's rint is half-to-even)."""
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5).astype(np.int64)


def _decode(path, store_size):
    """One image -> HWC uint8 RGB, shorter side at most ``store_size``."""
    from PIL import Image
    with Image.open(path) as im:
        if im.format == 'JPEG':
            w, h = im.size
            short = min(w, h)
            if short > store_size:
                # DCT-domain downscale to the smallest size still >= target
                im.draft('RGB', (int(math.ceil(w * store_size / short)),
                                 int(math.ceil(h * store_size / short))))
        im = im.convert('RGB')
        w, h = im.size
        short = min(w, h)
        if short > store_size:  # never upsample
            nw = max(1, int(_round(w * store_size / short)))
            nh = max(1, int(_round(h * store_size / short)))
            im = im.resize((nw, nh), Image.BILINEAR)
        return np.asarray(im, dtype=np.uint8)


class ImageStore:
    """A folder of class sub-directories, decoded once into a byte arena.

    ``arena`` is a 1-D uint8 tensor holding every image HWC RGB back to
    back; ``offsets``/``H``/``W``/``labels`` are host numpy index arrays.

    ``store_device``: 'cuda' keeps the arena in HBM (no host image traffic
    in the steady state); 'host' keeps it in pinned memory and stages each
    batch's images through one non-blocking upload; 'auto' picks 'cuda' when
    the arena fits in half of the free device memory, 'host' otherwise or
    when there is no GPU.
    """

    def __init__(self, root, store_size=256, device=None, workers=10,
                 cache=None, store_device='auto'):
        if store_device not in ('auto', 'cuda', 'host'):
            raise ValueError("store_device must be 'auto', 'cuda' or 'host'")
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.device = torch.device(device)
        self.root = root
        self.store_size = int(store_size)
        samples, class_to_idx = find_images_and_targets(root)
        if not samples:
            raise RuntimeError('Found 0 images in %s' % root)
        self.classes = [c for c, _ in sorted(class_to_idx.items(),
                                             key=lambda kv: kv[1])]
        self.filenames = [f for f, _ in samples]

        loaded = self._load_cache(cache, len(samples)) if cache else None
        self.from_cache = loaded is not None
        if loaded is None:
            arena, index = self._decode_all(samples, workers)
            if cache:
                self._write_cache(cache, arena, index)
        else:
            arena, index = loaded
        self._adopt(arena, index, store_device)

    @classmethod
    def from_arrays(cls, arena, index, classes, store_size=256, device=None,
                    store_device='auto'):
        """A store over an already packed uint8 ``arena`` and its int64
        ``index`` [N, 4] = (offset, H, W, label): synthetic data, no files."""
        if store_device not in ('auto', 'cuda', 'host'):
            raise ValueError("store_device must be 'auto', 'cuda' or 'host'")
        self = cls.__new__(cls)
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.device = torch.device(device)
        self.root = None
        self.store_size = int(store_size)
        self.classes = list(classes)
        self.filenames = []
        self.from_cache = False
        self._adopt(arena, index, store_device)
        return self

    def _adopt(self, arena, index, store_device):
        self.offsets = np.ascontiguousarray(index[:, 0])
        self.H = index[:, 1].astype(np.int32)
        self.W = index[:, 2].astype(np.int32)
        self.labels = np.ascontiguousarray(index[:, 3])
        self._place(arena, store_device)

    # -- decode / pack ------------------------------------------------------

    def _decode_all(self, samples, workers):
        n_threads = max(1, min(int(workers), _MAX_WORKERS))
        size = self.store_size
        with ThreadPoolExecutor(n_threads) as pool:
            images = list(pool.map(lambda s: _decode(s[0], size), samples))
        index = np.zeros((len(samples), 4), dtype=np.int64)
        pos = 0
        for i, (img, (_, label)) in enumerate(zip(images, samples)):
            index[i] = (pos, img.shape[0], img.shape[1], label)
            pos += img.size
        arena = np.empty(pos, dtype=np.uint8)
        for i, img in enumerate(images):
            arena[index[i, 0]:index[i, 0] + img.size] = img.reshape(-1)
            images[i] = None
        return arena, index

    # -- cache (this project's own format) -----------------------------------

    @staticmethod
    def _cache_paths(cache):
        return (os.path.join(cache, 'arena.npy'),
                os.path.join(cache, 'index.npy'),
                os.path.join(cache, 'store.json'))

    def _load_cache(self, cache, count):
        arena_p, index_p, info_p = self._cache_paths(cache)
        if not all(os.path.isfile(p) for p in (arena_p, index_p, info_p)):
            return None
        with open(info_p) as f:
            info = json.load(f)
        if (info.get('version') != _CACHE_VERSION
                or info.get('count') != count
                or info.get('store_size') != self.store_size
                or info.get('classes') != self.classes):
            return None
        index = np.load(index_p)
        arena = np.load(arena_p)
        if index.shape != (count, 4) or arena.dtype != np.uint8 \
                or arena.size != info.get('bytes'):
            return None
        return arena, index

    def _write_cache(self, cache, arena, index):
        os.makedirs(cache, exist_ok=True)
        arena_p, index_p, info_p = self._cache_paths(cache)
        np.save(arena_p, arena)
        np.save(index_p, index)
        with open(info_p, 'w') as f:  # written last: marks the cache whole
            json.dump({'version': _CACHE_VERSION, 'count': int(len(index)),
                       'store_size': self.store_size,
                       'bytes': int(arena.size), 'classes': self.classes}, f)

    # -- placement ----------------------------------------------------------

    def _place(self, arena, store_device):
        on_gpu = self.device.type == 'cuda'
        if store_device == 'cuda' and not on_gpu:
            raise RuntimeError("store_device='cuda' needs a GPU device")
        if store_device == 'auto':
            if on_gpu:
                free, _ = torch.cuda.mem_get_info(self.device)
                store_device = 'cuda' if arena.size <= free // 2 else 'host'
            else:
                store_device = 'host'
        self.store_device = store_device
        t = torch.from_numpy(arena)
        if store_device == 'cuda':
            self.arena = t.to(self.device)
        elif on_gpu:
            self.arena = t.pin_memory()
        else:
            self.arena = t

    def __len__(self):
        return len(self.labels)

    @property
    def nbytes(self):
        return int(self.arena.numel())

    # -- one batch ------------------------------------------------------------

    def batch(self, idx, meta, size, mean, std, dtype):
        """Run the fused op for samples ``idx`` with geometry ``meta``
        (int32[B, 11], columns H..flip already filled). Returns
        (images [B,3,S,S] channels_last, target int64[B]) on ``device``."""
        targets = np.ascontiguousarray(self.labels[idx])
        if self.device.type != 'cuda':
            images = ops.crop_resize_mirror_normalize(
                self.arena, np.ascontiguousarray(self.offsets[idx]), meta,
                size, mean, std, dtype)
            return images, torch.from_numpy(targets)

        if self.store_device == 'cuda':
            arena = self.arena
            offsets = np.ascontiguousarray(self.offsets[idx])
        else:
            # pack this batch's images into pinned staging, one upload
            nbytes = 3 * self.H[idx].astype(np.int64) * self.W[idx]
            offsets = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
            staging = torch.empty(int(nbytes.sum()), dtype=torch.uint8,
                                  pin_memory=True)
            src = self.offsets[idx]
            torch.cat([self.arena[o:o + n] for o, n in
                       zip(src.tolist(), nbytes.tolist())], out=staging)
            arena = staging.to(self.device, non_blocking=True)
        off_d, meta_d, target = ops.functional.upload_crop_request(
            offsets, meta, self.device, targets=targets)
        images = ops.crop_resize_mirror_normalize(
            arena, off_d, meta_d, size, mean, std, dtype,
            host_copies=(offsets, meta))
        return images, target


def random_resized_boxes(H, W, rng, scale=(0.1, 1.0), ratio=(0.8, 1.25),
                         attempts=10, return_fallback=False):
    """Random-resized-crop boxes for a batch, vectorised.

    Area is uniform in ``scale * H * W`` and aspect (w/h) log-uniform in
    ``ratio`` (the reference DALI pipeline's ranges, utils.py:74-75);
    ``w = round(sqrt(area * ar))``, ``h = round(sqrt(area / ar))``; the first
    of ``attempts`` draws that fits the image wins. Samples with no fitting
    draw get the largest centred box whose aspect is clamped into ``ratio``.
    Returns int32 arrays (x0, y0, bw, bh) [, fallback mask].
    """
    H = np.asarray(H, dtype=np.int64)
    W = np.asarray(W, dtype=np.int64)
    n = H.shape[0]
    bw = np.zeros(n, dtype=np.int64)
    bh = np.zeros(n, dtype=np.int64)
    done = np.zeros(n, dtype=bool)
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(attempts):
        # full-batch draws every attempt keep the stream seed-deterministic
        area = rng.uniform(scale[0], scale[1], n) * H * W
        ar = np.exp(rng.uniform(log_lo, log_hi, n))
        w = _round(np.sqrt(area * ar))
        h = _round(np.sqrt(area / ar))
        take = ~done & (w >= 1) & (h >= 1) & (w <= W) & (h <= H)
        bw[take] = w[take]
        bh[take] = h[take]
        done |= take
    fell = ~done
    if fell.any():
        in_ratio = W / H
        fw = np.where(in_ratio > ratio[1], _round(H * ratio[1]), W)
        fh = np.where(in_ratio < ratio[0], _round(W / ratio[0]), H)
        bw[fell] = np.clip(fw, 1, W)[fell]
        bh[fell] = np.clip(fh, 1, H)[fell]
    x0 = rng.integers(0, W - bw + 1)
    y0 = rng.integers(0, H - bh + 1)
    x0[fell] = ((W - bw) // 2)[fell]
    y0[fell] = ((H - bh) // 2)[fell]
    out = tuple(a.astype(np.int32) for a in (x0, y0, bw, bh))
    return out + (fell,) if return_fallback else out


def center_boxes(H, W, S, resize=None):
    """Validation geometry: the whole image resized so its shorter side is
    ``resize`` (default ``round(S / 0.875)``, 256 for 224; the longer side is
    rounded), then the centred S x S window. Returns int32 arrays
    (x0, y0, bw, bh, oh, ow, oy, ox)."""
    H = np.asarray(H, dtype=np.int64)
    W = np.asarray(W, dtype=np.int64)
    if resize is None:
        resize = int(_round(S / 0.875))
    if resize < S:
        raise ValueError('resize (%d) must be >= the crop size (%d)'
                         % (resize, S))
    short = np.minimum(H, W)
    oh = np.where(H <= W, resize, _round(H * resize / short))
    ow = np.where(W <= H, resize, _round(W * resize / short))
    oy = (oh - S) // 2
    ox = (ow - S) // 2
    zero = np.zeros_like(H)
    return tuple(a.astype(np.int32)
                 for a in (zero, zero, W, H, oh, ow, oy, ox))


class GPUImageLoader:
    """Iterable of ``(images, target)`` batches over an ``ImageStore``.

    Train: seeded per-epoch permutation, drop_last, random-resized boxes and
    a per-sample coin-flip mirror. Val: natural order, last partial batch
    kept, centre boxes, no mirror. Ranks take the static shard
    ``indices[rank::world_size]``. Each step computes the batch geometry on
    the host, uploads it once (non-blocking) and calls the fused op; there
    is no ``.item()`` and no device-to-host copy in the loop.
    """

    def __init__(self, store, batch_size, size=224, train=True,
                 dtype=torch.float32, mean=(0.0, 0.0, 0.0),
                 std=(1.0, 1.0, 1.0), seed=0, rank=0, world_size=1,
                 resize=None):
        self.store = store
        self.batch_size = int(batch_size)
        self.size = int(size)
        self.train = bool(train)
        self.dtype = dtype
        self.mean = tuple(mean)
        self.std = tuple(std)
        self.seed = int(seed)
        self.rank = int(rank)
        self.world_size = int(world_size)
        self.resize = resize
        self.epoch = 0
        self._count = len(range(self.rank, len(store), self.world_size))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        if self.train:
            return self._count // self.batch_size
        return -(-self._count // self.batch_size)

    def index_batches(self):
        """The store indices of every batch of the current epoch."""
        order = np.arange(len(self.store))
        if self.train:
            order = np.random.default_rng(
                [self.seed, self.epoch]).permutation(order)
        order = order[self.rank::self.world_size]
        B = self.batch_size
        return [order[i * B:(i + 1) * B] for i in range(len(self))]

    def __iter__(self):
        S = self.size
        store = self.store
        rng = np.random.default_rng([self.seed, self.epoch, self.rank, 1])
        for idx in self.index_batches():
            H, W = store.H[idx], store.W[idx]
            meta = np.zeros((len(idx), 11), dtype=np.int32)
            meta[:, 0], meta[:, 1] = H, W
            if self.train:
                x0, y0, bw, bh = random_resized_boxes(H, W, rng)
                meta[:, 2], meta[:, 3], meta[:, 4], meta[:, 5] = x0, y0, bw, bh
                meta[:, 6] = S
                meta[:, 7] = S
                meta[:, 10] = rng.integers(0, 2, len(idx))
            else:
                for c, col in enumerate(center_boxes(H, W, S, self.resize)):
                    meta[:, 2 + c] = col
            yield store.batch(idx, meta, S, self.mean, self.std, self.dtype)
