"""Image-folder pipeline on the CPU: sampling rule and oracle, host-side
validation, box samplers, the decoded store and its cache, the loader's
sharding/shuffling, and the ImageNet driver trained from a folder.

Every image is generated from a seed into tmp_path.
"""

import math
import os

import numpy as np
import pytest
import torch

from noisynet_amd import data as data_mod
from noisynet_amd import image_pipeline as ip
from noisynet_amd import ops
from noisynet_amd.drivers import imagenet

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# class dirs and file names chosen so natural order != lexical order
# (c1 < c2 < c10, img2 < img10). (name, H, W, mode)
TREE = {
    'c2': [('img1.png', 40, 64, 'RGB'), ('img2.png', 17, 23, 'RGB'),
           ('img10.png', 32, 45, 'RGB'), ('img11.png', 50, 33, 'RGB')],
    'c10': [('img1.png', 25, 25, 'RGB'), ('img2.png', 64, 64, 'RGB'),
            ('img10.png', 31, 70, 'RGB'), ('img3.png', 36, 36, 'RGB')],
    'c1': [('img1.png', 37, 53, 'RGB'), ('img2.png', 20, 30, 'L'),
           ('img10.png', 48, 40, 'RGBA'), ('img3.jpg', 60, 80, 'RGB')],
}
NATURAL_CLASSES = ['c1', 'c2', 'c10']


def make_tree(root, seed=0):
    """Write the 3-class x 4-image tree under ``root``."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for cls, files in TREE.items():
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for name, h, w, mode in files:
            ch = {'RGB': 3, 'L': 1, 'RGBA': 4}[mode]
            if name.endswith('.jpg'):
                # smooth content so JPEG artefacts stay small
                yy, xx = np.mgrid[0:h, 0:w]
                a = np.stack([yy * 3, xx * 2, yy + xx], -1) % 256
            else:
                a = rng.randint(0, 256, (h, w, ch))
            a = a.astype(np.uint8)
            Image.fromarray(a[..., 0] if ch == 1 else a, mode=mode).save(
                os.path.join(root, cls, name))
    return root


def make_dataset(tmp_path, val=True):
    make_tree(str(tmp_path / 'train'), seed=0)
    if val:
        make_tree(str(tmp_path / 'val'), seed=1)
    return str(tmp_path)


def one_meta(H, W, box, virt, win, flip):
    return np.array([[H, W, box[0], box[1], box[2], box[3], virt[0], virt[1],
                      win[0], win[1], flip]], dtype=np.int32)


def run_one(img, meta, S, **kw):
    arena = torch.from_numpy(np.ascontiguousarray(img)).reshape(-1)
    return ops.crop_resize_mirror_normalize(
        arena, np.zeros(1, dtype=np.int64), meta, S, **kw)


# ---------------------------------------------------------------------------
# rule and oracle
# ---------------------------------------------------------------------------

def hand_weights(n_in, n_out, o):
    """The issue's per-axis rule, in float64."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    center = scale * (o + 0.5)
    lo = max(0, int(center - fs + 0.5))
    hi = min(n_in, int(center + fs + 0.5))
    w = np.zeros(n_in)
    for j in range(lo, hi):
        w[j] = max(0.0, 1.0 - abs((j - center + 0.5) / fs))
    return w / w.sum()


def test_hand_weights_are_the_expected_fractions():
    # 4 -> 2: taps (3, 3, 1)/7 and mirrored; 2 -> 4: (1,0) (.75,.25) ...
    assert np.allclose(hand_weights(4, 2, 0), [3 / 7, 3 / 7, 1 / 7, 0])
    assert np.allclose(hand_weights(4, 2, 1), [0, 1 / 7, 3 / 7, 3 / 7])
    assert np.allclose(hand_weights(2, 4, 0), [1, 0])
    assert np.allclose(hand_weights(2, 4, 1), [0.75, 0.25])
    assert np.allclose(hand_weights(2, 4, 2), [0.25, 0.75])
    assert np.allclose(hand_weights(2, 4, 3), [0, 1])


@pytest.mark.parametrize('n_in,n_out', [(4, 2), (2, 4)])
def test_reference_op_matches_hand_computed(n_in, n_out):
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (n_in, n_in, 3)).astype(np.uint8)
    out = run_one(img, one_meta(n_in, n_in, (0, 0, n_in, n_in),
                                (n_out, n_out), (0, 0), 0), n_out)
    Wm = np.stack([hand_weights(n_in, n_out, o) for o in range(n_out)])
    want = np.einsum('yi,xj,ijc->cyx', Wm, Wm, img.astype(np.float64) / 255)
    assert out.shape == (1, 3, n_out, n_out)
    assert np.abs(out[0].numpy() - want).max() < 1e-6


def test_identity_and_mirror_are_exact():
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (16, 16, 3)).astype(np.uint8)
    want = torch.from_numpy(img).permute(2, 0, 1).float() / 255.0
    out = run_one(img, one_meta(16, 16, (0, 0, 16, 16), (16, 16), (0, 0), 0),
                  16)
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out[0], want)
    out = run_one(img, one_meta(16, 16, (0, 0, 16, 16), (16, 16), (0, 0), 1),
                  16)
    assert torch.equal(out[0], want.flip(-1))


def test_normalisation():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    meta = one_meta(37, 53, (5, 3, 40, 29), (16, 16), (0, 0), 1)
    raw = run_one(img, meta, 16)
    out = run_one(img, meta, 16, mean=MEAN, std=STD)
    want = (raw - torch.tensor(MEAN).view(1, 3, 1, 1)) \
        / torch.tensor(STD).view(1, 3, 1, 1)
    assert (out - want).abs().max() <= 1e-6
    for dt in (torch.bfloat16, torch.float16):
        o = run_one(img, meta, 16, out_dtype=dt)
        assert o.dtype == dt and torch.equal(o, raw.to(dt))


# ---------------------------------------------------------------------------
# host-side validation (no launch)
# ---------------------------------------------------------------------------

GOOD = dict(H=10, W=12, box=(2, 1, 8, 7), virt=(6, 9), win=(1, 2), flip=0)


def _request(**over):
    d = dict(GOOD)
    d.update(over)
    return one_meta(d['H'], d['W'], d['box'], d['virt'], d['win'], d['flip'])


@pytest.mark.parametrize('over', [
    dict(box=(-1, 1, 8, 7)),          # x0 < 0
    dict(box=(5, 1, 8, 7)),           # x0 + bw > W
    dict(box=(2, -1, 8, 7)),          # y0 < 0
    dict(box=(2, 4, 8, 7)),           # y0 + bh > H
    dict(box=(2, 1, 0, 7)),           # bw < 1
    dict(box=(2, 1, 8, 0)),           # bh < 1
    dict(win=(3, 2)),                 # window leaves oh (3 + 4 > 6)
    dict(win=(1, 6)),                 # window leaves ow (6 + 4 > 9)
    dict(win=(-1, 2)),
    dict(virt=(3, 9)),                # virtual image smaller than S
    dict(flip=2),
], ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_malformed_requests_raise(over):
    arena = torch.zeros(3 * 10 * 12, dtype=torch.uint8)
    off = np.zeros(1, dtype=np.int64)
    ops.crop_resize_mirror_normalize(arena, off, _request(), 4)  # baseline ok
    with pytest.raises(ValueError):
        ops.crop_resize_mirror_normalize(arena, off, _request(**over), 4)


def test_malformed_arena_offsets_dtypes_raise():
    arena = torch.zeros(3 * 10 * 12, dtype=torch.uint8)
    off = np.zeros(1, dtype=np.int64)
    meta = _request()
    bad = [
        (arena, np.array([1], dtype=np.int64), meta, 4),      # past the end
        (arena, np.array([-1], dtype=np.int64), meta, 4),
        (arena[:-1], off, meta, 4),                           # arena short
        (arena, off, meta, 0),                                # S < 1
        (arena, off.astype(np.int32), meta, 4),               # offsets dtype
        (arena, off, meta.astype(np.int64), 4),               # meta dtype
        (arena.float(), off, meta, 4),                        # arena dtype
        (arena, off, meta[:, :10], 4),                        # meta shape
        (arena, np.zeros(2, dtype=np.int64), meta, 4),        # B mismatch
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.crop_resize_mirror_normalize(*args)
    with pytest.raises(ValueError):
        ops.crop_resize_mirror_normalize(arena, off, meta, 4,
                                         out_dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.crop_resize_mirror_normalize(arena, off, meta, 4,
                                         std=(1.0, 0.0, 1.0))


# ---------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------

def _mixed_sizes(n, seed):
    r = np.random.RandomState(seed)
    return r.randint(30, 400, n), r.randint(30, 400, n)


def test_random_boxes_inside_and_in_range():
    H, W = _mixed_sizes(10000, 0)
    x0, y0, bw, bh, fell = ip.random_resized_boxes(
        H, W, np.random.default_rng(7), return_fallback=True)
    assert (x0 >= 0).all() and (y0 >= 0).all()
    assert (bw >= 1).all() and (bh >= 1).all()
    assert (x0 + bw <= W).all() and (y0 + bh <= H).all()
    ok = ~fell
    assert ok.sum() > 9000
    bw_, bh_ = bw[ok].astype(np.float64), bh[ok].astype(np.float64)
    area = (H * W)[ok]
    # w, h are within 0.5 of the real-valued draw: propagate that rounding
    lo_area = (bw_ - 0.5).clip(0) * (bh_ - 0.5).clip(0) / area
    hi_area = (bw_ + 0.5) * (bh_ + 0.5) / area
    assert (hi_area >= 0.1).all() and (lo_area <= 1.0).all()
    assert ((bw_ + 0.5) / (bh_ - 0.5).clip(1e-9) >= 0.8).all()
    assert ((bw_ - 0.5) / (bh_ + 0.5) <= 1.25).all()
    # the whole scale range is used, not a corner of it
    frac = bw_ * bh_ / area
    assert frac.min() < 0.15 and frac.max() > 0.9


def test_random_boxes_seeded():
    H, W = _mixed_sizes(10000, 1)
    a = ip.random_resized_boxes(H, W, np.random.default_rng(11))
    b = ip.random_resized_boxes(H, W, np.random.default_rng(11))
    c = ip.random_resized_boxes(H, W, np.random.default_rng(12))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert any(not np.array_equal(p, q) for p, q in zip(a, c))
    assert all(p.dtype == np.int32 for p in a)


def test_random_boxes_fallback():
    n = 1000
    H, W = np.full(n, 8), np.full(n, 200)
    x0, y0, bw, bh, fell = ip.random_resized_boxes(
        H, W, np.random.default_rng(0), return_fallback=True)
    assert fell.all()                       # 100 % fallback
    assert (bh == 8).all() and (bw == 10).all()   # aspect clamped to 1.25
    assert (x0 == 95).all() and (y0 == 0).all()   # centred, inside
    # the transposed image clamps at the other end of the range
    x0, y0, bw, bh, fell = ip.random_resized_boxes(
        W, H, np.random.default_rng(0), return_fallback=True)
    assert fell.all() and (bw == 8).all() and (bh == 10).all()
    assert (y0 == 95).all() and (x0 == 0).all()

    H, W = np.full(n, 256), np.full(n, 341)
    *_, fell = ip.random_resized_boxes(H, W, np.random.default_rng(0),
                                       return_fallback=True)
    assert fell.mean() < 0.01


def test_center_boxes():
    x0, y0, bw, bh, oh, ow, oy, ox = ip.center_boxes([256], [341], 224, 256)
    assert (x0[0], y0[0], bw[0], bh[0]) == (0, 0, 341, 256)
    assert (oh[0], ow[0]) == (256, 341)
    assert (oy[0], ox[0]) == (16, 58)
    # default resize = round(S / 0.875); portrait and upscaled inputs
    *_, oh, ow, oy, ox = ip.center_boxes([500, 30], [375, 30], 224)
    assert (oh[0], ow[0]) == (341, 256) and (oy[0], ox[0]) == (58, 16)
    assert (oh[1], ow[1]) == (256, 256) and (oy[1], ox[1]) == (16, 16)


# ---------------------------------------------------------------------------
# store
# ---------------------------------------------------------------------------

def _stored(store, i):
    o, h, w = int(store.offsets[i]), int(store.H[i]), int(store.W[i])
    return store.arena[o:o + 3 * h * w].view(h, w, 3).cpu().numpy()


def test_store_contents(tmp_path):
    from PIL import Image
    root = make_tree(str(tmp_path / 'train'))
    store = ip.ImageStore(root, store_size=32, device='cpu', workers=4)
    assert len(store) == 12
    assert store.classes == NATURAL_CLASSES
    assert store.store_device == 'host' and store.arena.dtype == torch.uint8
    assert store.nbytes == int((3 * store.H.astype(np.int64) * store.W).sum())

    # natural order: classes c1, c2, c10; files img1, img2, ..., img10
    rel = [os.path.relpath(f, root) for f in store.filenames]
    assert rel[:4] == ['c1/img1.png', 'c1/img2.png', 'c1/img3.jpg',
                       'c1/img10.png']
    assert rel[4:8] == ['c2/img1.png', 'c2/img2.png', 'c2/img10.png',
                        'c2/img11.png']
    assert store.labels.tolist() == [0] * 4 + [1] * 4 + [2] * 4

    exact = 0
    for i, f in enumerate(store.filenames):
        src = np.asarray(Image.open(f).convert('RGB'))
        h, w = src.shape[:2]
        got = _stored(store, i)
        if min(h, w) <= 32:     # never upsampled, stored as is
            assert got.shape == src.shape
            if f.endswith('.png'):
                assert np.array_equal(got, src), f
                exact += 1
        else:
            assert min(got.shape[:2]) == 32
    assert exact == 5
    by_name = {r: _stored(store, i).shape for i, r in enumerate(rel)}
    assert by_name['c2/img1.png'] == (32, 51, 3)      # 40x64 at store_size 32
    assert by_name['c1/img3.jpg'] == (32, 43, 3)      # the JPEG, 60x80
    assert by_name['c1/img2.png'] == (20, 30, 3)      # grayscale -> RGB
    g = _stored(store, rel.index('c1/img2.png'))
    assert np.array_equal(g[..., 0], g[..., 1])
    assert by_name['c1/img10.png'] == (38, 32, 3)     # RGBA 48x40 -> RGB

    # a JPEG small enough to be kept decodes to its own shape
    keep = ip.ImageStore(root, store_size=64, device='cpu')
    assert _stored(keep, rel.index('c1/img3.jpg')).shape == (60, 80, 3)


def test_store_cache_roundtrip(tmp_path):
    root = make_tree(str(tmp_path / 'train'))
    cache = str(tmp_path / 'cache')
    a = ip.ImageStore(root, store_size=32, device='cpu', cache=cache)
    assert not a.from_cache
    b = ip.ImageStore(root, store_size=32, device='cpu', cache=cache)
    assert b.from_cache
    assert torch.equal(a.arena, b.arena)
    for name in ('offsets', 'H', 'W', 'labels'):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a.classes == b.classes
    # another store_size must not reuse it
    c = ip.ImageStore(root, store_size=40, device='cpu', cache=cache)
    assert not c.from_cache
    assert c.nbytes != a.nbytes
    # ... and a changed file count neither
    os.remove(os.path.join(root, 'c2', 'img11.png'))
    d = ip.ImageStore(root, store_size=40, device='cpu', cache=cache)
    assert not d.from_cache and len(d) == 11


# ---------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cpu_store(tmp_path_factory):
    root = make_tree(str(tmp_path_factory.mktemp('tree') / 'train'))
    return ip.ImageStore(root, store_size=40, device='cpu')


def test_val_loader_shards_cover_everything(cpu_store):
    seen = []
    for rank in range(2):
        ld = ip.GPUImageLoader(cpu_store, 4, size=32, train=False, rank=rank,
                               world_size=2)
        batches = ld.index_batches()
        assert len(ld) == 2 and [len(b) for b in batches] == [4, 2]
        out = list(ld)
        assert [x.shape[0] for x, _ in out] == [4, 2]   # partial batch kept
        for idx, (x, y) in zip(batches, out):
            assert x.shape[1:] == (3, 32, 32)
            assert y.tolist() == cpu_store.labels[idx].tolist()
        seen += np.concatenate(batches).tolist()
    assert sorted(seen) == list(range(12))
    # natural order, no shuffling, no mirror: deterministic
    ld = ip.GPUImageLoader(cpu_store, 5, size=32, train=False)
    assert np.concatenate(ld.index_batches()).tolist() == list(range(12))
    a, b = list(ld), list(ld)
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a, b))


def test_train_loader(cpu_store):
    ld = ip.GPUImageLoader(cpu_store, 5, size=32, train=True,
                           dtype=torch.bfloat16, seed=3)
    assert len(ld) == 2                                  # drop_last
    ld.set_epoch(0)
    e0 = np.concatenate(ld.index_batches())
    b0 = list(ld)
    ld.set_epoch(1)
    e1 = np.concatenate(ld.index_batches())
    assert len(e0) == 10 and len(set(e0.tolist())) == 10   # at most once
    assert len(set(e1.tolist())) == 10
    assert e0.tolist() != e1.tolist()
    for x, y in b0:
        assert x.shape == (5, 3, 32, 32) and x.dtype == torch.bfloat16
        assert x.is_contiguous(memory_format=torch.channels_last)
        assert y.shape == (5,) and y.dtype == torch.int64
    assert torch.cat([y for _, y in b0]).tolist() == \
        cpu_store.labels[e0].tolist()

    again = ip.GPUImageLoader(cpu_store, 5, size=32, train=True,
                              dtype=torch.bfloat16, seed=3)
    again.set_epoch(0)
    for (x, y), (x2, y2) in zip(b0, again):
        assert torch.equal(x, x2) and torch.equal(y, y2)
    other = ip.GPUImageLoader(cpu_store, 5, size=32, train=True,
                              dtype=torch.bfloat16, seed=4)
    assert np.concatenate(other.index_batches()).tolist() != e0.tolist()

    # two ranks of a training epoch are disjoint
    r = [np.concatenate(ip.GPUImageLoader(
        cpu_store, 3, size=32, train=True, seed=3, rank=k,
        world_size=2).index_batches()).tolist() for k in range(2)]
    assert not set(r[0]) & set(r[1]) and len(r[0]) == len(r[1]) == 6


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------

def driver_argv(data, extra=()):
    return ['--data', data, '-a', 'resnet18', '--image_size', '32',
            '--store_size', '40', '-b', '4', '--epochs', '1', '-p', '1',
            '-j', '4'] + list(extra)


def check_driver_output(text, tmp_path):
    import re
    losses = [float(v) for v in re.findall(r'loss ([-+.\w]+)', text)]
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    acc = re.findall(r'Epoch 0 val acc ([\d.]+)', text)
    assert len(acc) == 1 and 0.0 <= float(acc[0]) <= 100.0
    assert '12 train / 12 val images, 3 classes' in text
    ckpt = tmp_path / 'results' / 'resnet18' / 'checkpoint.pth.tar'
    assert ckpt.is_file()


def test_driver_trains_from_folder(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    data = make_dataset(tmp_path / 'data')
    imagenet.main(driver_argv(data))
    check_driver_output(capsys.readouterr().out, tmp_path)


def test_driver_without_val_folder(tmp_path, capsys):
    data = make_dataset(tmp_path / 'data', val=False)
    args = imagenet.build_main_parser().parse_args(driver_argv(data))
    train_loader, val_loader = imagenet.setup_data(args, torch.device('cpu'))
    assert val_loader.store is train_loader.store and not val_loader.train
    assert capsys.readouterr().out.count('no val folder') == 1
    assert sum(x.shape[0] for x, _ in val_loader) == 12


def test_driver_missing_path_stays_synthetic(tmp_path):
    args = imagenet.build_main_parser().parse_args(
        ['--data', str(tmp_path / 'nowhere'), '-b', '2',
         '--synthetic_batches', '3'])
    loaders = imagenet.setup_data(args, torch.device('cpu'))
    assert all(isinstance(ld, data_mod.SyntheticImageNet) for ld in loaders)
    assert len(loaders[0]) == 3
    # the defaults of the new flags change nothing
    d = imagenet.build_main_parser().parse_args([])
    assert (d.image_size, d.store_size, d.store_device, d.data_cache,
            d.imagenet_norm) == (224, 256, 'auto', None, False)
    assert not os.path.isdir(os.path.join(d.data, 'train'))
