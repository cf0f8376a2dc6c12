"""The fused crop/resize/mirror/normalise HIP kernel against the fp32 CPU
oracle (the per-sample ``F.interpolate(antialias=True)`` composition in
ops/reference.py), plus the loader and driver on the GPU.

Expected values never come from the kernel. Tolerances: fp32 within 2e-5
absolute before normalisation (weights sum to 1, values in [0, 1], so the
error is bounded by taps * 2^-24; the largest case has < 200 taps -> 1.2e-5);
bf16/fp16 within one unit in the last place of ``oracle.to(dtype)``.
"""

import numpy as np
import pytest
import torch

from noisynet_amd import image_pipeline as ip
from noisynet_amd import ops
from noisynet_amd.drivers import imagenet
from noisynet_amd.ops import reference as ref

from test_image_pipeline import (check_driver_output, driver_argv,
                                 make_dataset, make_tree)

pytestmark = pytest.mark.gpu

S = 16
# (H, W), box (x0, y0, bw, bh), virtual (oh, ow), window (oy, ox), flip
SWEEP = [
    ((37, 53), (5, 3, 40, 29), (16, 16), (0, 0), 0),
    ((37, 53), (0, 0, 53, 37), (16, 23), (0, 3), 1),
    ((9, 7), (1, 2, 5, 6), (16, 16), (0, 0), 1),
    ((130, 97), (0, 0, 97, 130), (21, 16), (2, 0), 0),
    ((16, 16), (0, 0, 16, 16), (16, 16), (0, 0), 0),     # identity
    ((3, 2), (1, 2, 1, 1), (16, 16), (0, 0), 0),         # 1x1 box
    ((1, 1), (0, 0, 1, 1), (16, 16), (0, 0), 0),
]


def pack(images, first=1):
    """Pack HWC uint8 images into one arena at offsets that are NOT
    multiples of 4 (random filler between them)."""
    rng = np.random.RandomState(99)
    chunks, offsets, pos = [], [], 0

    def fill(n):
        nonlocal pos
        chunks.append(rng.randint(0, 256, n).astype(np.uint8))
        pos += n

    fill(first)
    for img in images:
        if pos % 4 == 0:
            fill(1 + pos % 3)
        assert pos % 4 != 0
        offsets.append(pos)
        chunks.append(img.reshape(-1))
        pos += img.size
    fill(3)
    return (torch.from_numpy(np.concatenate(chunks)),
            np.array(offsets, dtype=np.int64))


@pytest.fixture(scope='module')
def sweep():
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, hw + (3,)).astype(np.uint8)
              for hw, *_ in SWEEP]
    arena, offsets = pack(images)
    meta = np.array([[hw[0], hw[1], *box, *virt, *win, flip]
                     for hw, box, virt, win, flip in SWEEP], dtype=np.int32)
    oracle = ref.crop_resize_mirror_normalize(
        arena, torch.from_numpy(offsets), torch.from_numpy(meta), S,
        (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.float32)
    return arena.cuda(), offsets, meta, oracle


@pytest.fixture(scope='module')
def realistic():
    rng = np.random.RandomState(1)
    # smooth + noise, like a photograph rather than white noise
    yy, xx = np.mgrid[0:300, 0:400]
    base = np.stack([yy * 0.6, xx * 0.5, (yy + xx) * 0.3], -1)
    img = (base + rng.randint(0, 80, (300, 400, 3))).clip(0, 255)
    img = img.astype(np.uint8)
    x0, y0, bw, bh = ip.random_resized_boxes(
        [300], [400], np.random.default_rng(5))
    meta = np.array([[300, 400, x0[0], y0[0], bw[0], bh[0], 224, 224, 0, 0,
                      1]], dtype=np.int32)
    arena, offsets = pack([img], first=3)
    oracle = ref.crop_resize_mirror_normalize(
        arena, torch.from_numpy(offsets), torch.from_numpy(meta), 224,
        (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.float32)
    return arena.cuda(), offsets, meta, oracle, 224


def ulp_distance(a, b):
    """Distance in units in the last place between two non-negative 16-bit
    float tensors (their bit patterns are monotonic for values >= 0)."""
    assert a.dtype == b.dtype and a.element_size() == 2
    assert (a >= 0).all() and (b >= 0).all()
    return (a.contiguous().view(torch.int16).int()
            - b.contiguous().view(torch.int16).int()).abs()


def check_against_oracle(arena, offsets, meta, oracle, size, dtype):
    out = ops.crop_resize_mirror_normalize(arena, offsets, meta, size,
                                           out_dtype=dtype)
    assert out.shape == oracle.shape and out.dtype == dtype
    assert out.is_cuda
    assert out.is_contiguous(memory_format=torch.channels_last)
    got = out.cpu()
    if dtype == torch.float32:
        err = (got - oracle).abs().amax(dim=(1, 2, 3))
        print('fp32 max abs error per sample:', err.tolist())
        assert err.max() <= 2e-5
    else:
        d = ulp_distance(got, oracle.to(dtype)).amax(dim=(1, 2, 3))
        print('%s max ulp distance per sample:' % dtype, d.tolist())
        assert d.max() <= 1
    return out


DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
def test_geometry_sweep(sweep, dtype):
    arena, offsets, meta, oracle = sweep
    assert (offsets % 4 != 0).all()
    out = check_against_oracle(arena, offsets, meta, oracle, S, dtype)
    again = ops.crop_resize_mirror_normalize(arena, offsets, meta, S,
                                             out_dtype=dtype)
    assert torch.equal(out, again)          # bit-identical relaunch
    if dtype == torch.float32:
        # identity sample: the stored pixels over 255
        o, n = int(offsets[4]), 16 * 16 * 3
        img = arena[o:o + n].view(16, 16, 3).permute(2, 0, 1).float().cpu()
        assert (out[4].cpu() - img / 255.0).abs().max() <= 2e-7


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16', 'fp16'])
def test_realistic_crop(realistic, dtype):
    arena, offsets, meta, oracle, size = realistic
    check_against_oracle(arena, offsets, meta, oracle, size, dtype)


def test_odd_output_size_takes_the_scalar_store_path(sweep):
    # S*S not a multiple of the 4 pixels a thread owns: tail + unaligned rows
    arena, offsets, meta, _ = sweep
    size = 15
    m = meta[:4].copy()
    oracle = ref.crop_resize_mirror_normalize(
        arena.cpu(), torch.from_numpy(offsets[:4]), torch.from_numpy(m),
        size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.float32)
    for dtype in DTYPES:
        check_against_oracle(arena, offsets[:4], m, oracle, size, dtype)


def test_normalisation_and_device_index_tensors(sweep):
    arena, offsets, meta, oracle = sweep
    mean, std = ip.IMAGENET_MEAN, ip.IMAGENET_STD
    out = ops.crop_resize_mirror_normalize(
        arena, torch.from_numpy(offsets).cuda(),
        torch.from_numpy(meta).cuda(), S, mean, std)
    want = (oracle - torch.tensor(mean).view(1, 3, 1, 1)) \
        / torch.tensor(std).view(1, 3, 1, 1)
    # 2e-5 on the [0, 1] value, scaled by 1/std
    assert (out.cpu() - want).abs().max() <= 2e-5 / min(std)


def test_offsets_past_2_31():
    rng = np.random.RandomState(2)
    img = torch.from_numpy(rng.randint(0, 256, 8 * 8 * 3).astype(np.uint8))
    meta = np.array([[8, 8, 1, 0, 7, 8, 16, 16, 0, 0, 1]], dtype=np.int32)
    small = ops.crop_resize_mirror_normalize(
        img.cuda(), np.zeros(1, dtype=np.int64), meta, S)
    big = torch.empty(2 ** 31 + 4096, dtype=torch.uint8, device='cuda')
    off = 2 ** 31 + 5
    big[off:off + img.numel()] = img.cuda()
    out = ops.crop_resize_mirror_normalize(
        big, np.array([off], dtype=np.int64), meta, S)
    assert torch.equal(out, small)
    oracle = ref.crop_resize_mirror_normalize(
        img, torch.zeros(1, dtype=torch.int64), torch.from_numpy(meta), S,
        (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.float32)
    assert (out.cpu() - oracle).abs().max() <= 2e-5


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(str(tmp_path_factory.mktemp('tree') / 'train'))


@pytest.mark.parametrize('train', [True, False], ids=['train', 'val'])
def test_loader_parity_across_placements(tree, train):
    stores = {
        'cpu': ip.ImageStore(tree, store_size=40, device='cpu'),
        'cuda': ip.ImageStore(tree, store_size=40, device='cuda',
                              store_device='cuda'),
        'host': ip.ImageStore(tree, store_size=40, device='cuda',
                              store_device='host'),
    }
    assert stores['cuda'].arena.is_cuda
    assert not stores['host'].arena.is_cuda
    assert stores['host'].arena.is_pinned()
    assert ip.ImageStore(tree, store_size=40,
                         device='cuda').store_device == 'cuda'   # auto
    got = {}
    for name, store in stores.items():
        ld = ip.GPUImageLoader(store, 5, size=32, train=train, seed=7)
        ld.set_epoch(2)
        got[name] = list(ld)
    assert len(got['cpu']) == (2 if train else 3)
    for (xc, yc), (xg, yg), (xh, yh) in zip(got['cpu'], got['cuda'],
                                            got['host']):
        assert xg.is_cuda and yg.is_cuda and xh.is_cuda
        assert xg.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(yg.cpu(), yc) and torch.equal(yh, yg)
        assert (xg.cpu() - xc).abs().max() <= 2e-5
        assert torch.equal(xh, xg)


def test_driver_trains_from_folder_bf16(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    data = make_dataset(tmp_path / 'data')
    seen = []
    build_model = imagenet.build_model

    def build_and_watch(args):
        built = build_model(args)
        built[0].register_forward_pre_hook(
            lambda mod, inputs: seen.append(
                (inputs[0].dtype, inputs[0].is_cuda, tuple(inputs[0].shape),
                 inputs[0].is_contiguous(memory_format=torch.channels_last))))
        return built

    monkeypatch.setattr(imagenet, 'build_model', build_and_watch)
    imagenet.main(driver_argv(data, ['--bf16']))
    check_driver_output(capsys.readouterr().out, tmp_path)
    assert len(seen) == 6           # 3 train steps + 3 val batches
    assert all(s == (torch.bfloat16, True, (4, 3, 32, 32), True)
               for s in seen)
