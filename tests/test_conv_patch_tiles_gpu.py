"""Layer-fitted block tiles of the image-patch conv (csrc/conv_mfma.hip).

The one-block-per-image tiles and their padding-row skip claim BIT-identity
with the 64x64 tile, not a tolerance: every output element is the same chain
of 16x16x32 MFMAs in (r, ck) order and the noise draw is keyed by
(image, 4-row group, channel). So each case runs the default tile choice and
``NOISYNET_PATCH_TILE=generic`` on the same inputs and seed and compares with
``torch.equal``. The noisy-forward tile is bit-identical too but measured
slower than the 64x64 tile on conv2 forward, so the default keeps it off; its
cases run it under ``NOISYNET_PATCH_TILE=all``. The plain conv is also held
to the fp64 oracle's deterministic bound (the generic tile skips no padding
rows, so equality alone already covers the skip; the reference is cheap).
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
from noisynet_amd import ops, utils  # noqa: E402
from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser  # noqa: E402
from noisynet_amd.models.noisynet import Net  # noqa: E402
from noisynet_amd.ops import functional as fn  # noqa: E402
from noisynet_amd.quant import finish_calibration, start_calibration  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
ENV = "NOISYNET_PATCH_TILE"
SEED = 123456789


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _tile(x_shape, w_shape, stride, pad, dtype, sigma_mode, telem=False):
    N, C, H, W = x_shape
    K, _, R, S = w_shape
    es = torch.empty(0, dtype=dtype).element_size()
    return ops.ext().conv_patch_tile(C, H, W, K, R, S, stride, pad, es,
                                     sigma_mode, telem)


def _empty(dtype):
    return torch.empty(0, device='cuda', dtype=dtype)


def _both(monkeypatch, call, fitted=None):
    """call() under the default tile choice (or under ``fitted``), then under
    the 64x64 tile."""
    if fitted is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, fitted)
    got = call()
    monkeypatch.setenv(ENV, "generic")
    want = call()
    monkeypatch.delenv(ENV, raising=False)
    return got, want


# ---------------------------------------------------------------------------
# conv2 forward geometry: 14x14x65 -> 120, 5x5, 100 pixels = 7 M-fragments
# ---------------------------------------------------------------------------

FWD_X, FWD_W = (3, 65, 14, 14), (120, 65, 5, 5)


def _fwd_inputs(dtype):
    inp = fo.make_inputs(FWD_X, FWD_W, dtype, seed=3)
    return (cl(inp.x.cuda()), cl(inp.wq.cuda()), cl(inp.w_raw.cuda()),
            inp.bias.cuda(), torch.tensor([0.5], device='cuda'))


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("sigma_mode", [1, 2], ids=["abs", "abs2"])
def test_conv2_forward_equals_generic(sigma_mode, with_bias, dtype,
                                      monkeypatch):
    x, wq, w_raw, bias, factor = _fwd_inputs(dtype)
    b = bias if with_bias else _empty(dtype)
    monkeypatch.setenv(ENV, "all")
    assert _tile(FWD_X, FWD_W, 1, 0, dtype, sigma_mode) == "7x8"

    def call():
        return ops.ext().conv_fwd_fused(x, wq, w_raw, b, 1, 0, sigma_mode,
                                        factor, SEED, False)[0]

    got, want = _both(monkeypatch, call, fitted="all")
    assert got.shape == (3, 120, 10, 10)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert bool((got != 0).any())
    assert torch.equal(got, want)


def test_env_switch_reports_generic(monkeypatch):
    monkeypatch.setenv(ENV, "generic")
    assert _tile(FWD_X, FWD_W, 1, 0, BF16, 2) == "generic"
    assert _tile((3, 120, 10, 10), (65, 120, 5, 5), 1, 4, BF16, 0) == "generic"
    monkeypatch.delenv(ENV)
    assert _tile((3, 120, 10, 10), (65, 120, 5, 5), 1, 4, BF16, 0) == "13x5"
    # the one-block noisy tile is opt-in (slower than 64x64 on conv2 forward)
    assert _tile(FWD_X, FWD_W, 1, 0, BF16, 2) == "generic"
    monkeypatch.setenv(ENV, "all")
    assert _tile(FWD_X, FWD_W, 1, 0, BF16, 2) == "7x8"
    assert _tile((3, 120, 10, 10), (65, 120, 5, 5), 1, 4, BF16, 0) == "13x5"
    # fp32 keeps the 64x64 tile; a layer off the patch route has no tile
    assert _tile(FWD_X, FWD_W, 1, 0, torch.float32, 2) == "generic"
    assert _tile((2, 3, 15, 15), (65, 3, 5, 5), 1, 0, BF16, 2) == "none"


@pytest.mark.parametrize("sigma_mode", [1, 2], ids=["abs", "abs2"])
def test_telemetry_takes_generic_tile_same_output(sigma_mode, monkeypatch):
    """The first 20 iterations run with telemetry (generic tile), the rest
    without (one-block tile where it is enabled): the switch must not move
    the output."""
    monkeypatch.setenv(ENV, "all")
    x, wq, w_raw, bias, factor = _fwd_inputs(BF16)
    assert _tile(FWD_X, FWD_W, 1, 0, BF16, sigma_mode, telem=True) == "generic"
    assert _tile(FWD_X, FWD_W, 1, 0, BF16, sigma_mode, telem=False) == "7x8"
    y_t, tele = ops.ext().conv_fwd_fused(x, wq, w_raw, bias, 1, 0, sigma_mode,
                                         factor, SEED, True)[:2]
    y = ops.ext().conv_fwd_fused(x, wq, w_raw, bias, 1, 0, sigma_mode,
                                 factor, SEED, False)[0]
    assert tele.numel() == 3 and float(tele[0]) > 0
    assert torch.equal(y, y_t)


# ---------------------------------------------------------------------------
# plain tile (SIGMA_MODE 0): conv2 dgrad geometry, tile edges, row skip
# ---------------------------------------------------------------------------


def _plain_inputs(x_shape, w_shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(x_shape, generator=g) * 0.5).to(dtype)
    w = (torch.randn(w_shape, generator=g) * 0.2).to(dtype)
    return x, w


def _plain_call(xg, wg, stride, pad):
    zero_f = torch.zeros(1, device='cuda', dtype=torch.float32)
    e = _empty(xg.dtype)

    def call():
        return ops.ext().conv_fwd_fused(xg, wg, wg, e, stride, pad, 0, zero_f,
                                        0, False)[0]
    return call


def _assert_fp64(got, x, w, stride, pad, dtype, what):
    ref = fo.to_mk(F.conv2d(x.double(), w.double(), None, stride, pad))
    A = fo.to_mk(F.conv2d(x.double().abs(), w.double().abs(), None, stride,
                          pad))
    n = w.shape[1] * w.shape[2] * w.shape[3] + w.shape[2] * w.shape[3]
    fo.assert_within(got, ref, fo.det_bound(ref, A, n, dtype), what)


def test_conv2_dgrad_equals_generic_and_fp64(monkeypatch):
    g_shape, w_shape = (3, 120, 10, 10), (120, 65, 5, 5)
    g, w = _plain_inputs(g_shape, w_shape, BF16, 5)
    gg, wg = cl(g.cuda()), cl(w.cuda())
    monkeypatch.delenv(ENV, raising=False)
    assert _tile(g_shape, (65, 120, 5, 5), 1, 4, BF16, 0) == "13x5"

    def call():
        return fn._conv_dgrad_raw(gg, wg, 1, 0, (3, 65, 14, 14))

    got, want = _both(monkeypatch, call)
    assert got.shape == (3, 65, 14, 14)
    assert torch.equal(got, want)
    ref = fo.to_mk(F.conv_transpose2d(g.double(), w.double()))
    A = fo.to_mk(F.conv_transpose2d(g.double().abs(), w.double().abs()))
    n = 120 * 25 + 25
    fo.assert_within(got, ref, fo.det_bound(ref, A, n, BF16), "conv2 dgrad")


# (x shape, w shape, stride, pad, expected tile, fp64 check too)
PLAIN_CASES = [
    # K edges of the <= 5 N-fragment tile on the dgrad geometry (pad 4 with
    # 5x5: 16 of 65 (fragment, row) pairs skipped); 81 must fall back
    ((2, 24, 10, 10), (1, 24, 5, 5), 1, 4, "13x1", True),
    ((2, 24, 10, 10), (16, 24, 5, 5), 1, 4, "13x1", False),
    ((2, 24, 10, 10), (17, 24, 5, 5), 1, 4, "13x2", False),
    ((2, 24, 10, 10), (79, 24, 5, 5), 1, 4, "13x5", False),
    ((2, 24, 10, 10), (80, 24, 5, 5), 1, 4, "13x5", True),
    ((2, 24, 10, 10), (81, 24, 5, 5), 1, 4, "generic", False),
    # MI = 1; MI = 16 exactly (fragments 1..15 lie wholly past MI); MI = 100
    ((2, 16, 5, 5), (20, 16, 5, 5), 1, 0, "1x2", True),
    ((2, 16, 8, 8), (20, 16, 5, 5), 1, 0, "1x2", True),
    ((2, 65, 14, 14), (40, 65, 5, 5), 1, 0, "7x3", True),
    # non-square, pad 1 with 3x3: few skipped pairs; MI = 60
    ((2, 65, 6, 10), (33, 65, 3, 3), 1, 1, "4x3", True),
    # ResNet-like 8x8x64 -> 64, 3x3 pad 1; C a multiple of 8, N = 1
    ((1, 64, 8, 8), (64, 64, 3, 3), 1, 1, "4x4", True),
    # C = 120, N = 1, MI = 196 with a 5-row tail fragment; stride 2
    ((1, 120, 10, 10), (65, 120, 5, 5), 1, 4, "13x5", True),
    ((3, 24, 15, 15), (20, 24, 3, 3), 2, 1, "4x2", True),
    # MI = 256: the largest the plain tile takes; 17x17 is past it
    ((1, 16, 16, 16), (20, 16, 3, 3), 1, 1, "16x2", True),
    ((1, 16, 17, 17), (20, 16, 3, 3), 1, 1, "generic", False),
]


@pytest.mark.parametrize("case", PLAIN_CASES,
                         ids=lambda c: "x".join(map(str, c[0])) + "-k%d-p%d"
                         % (c[1][0], c[3]))
def test_plain_tile_equals_generic(case, monkeypatch):
    x_shape, w_shape, stride, pad, tile, fp64 = case
    x, w = _plain_inputs(x_shape, w_shape, BF16, 7)
    monkeypatch.delenv(ENV, raising=False)
    assert _tile(x_shape, w_shape, stride, pad, BF16, 0) == tile
    got, want = _both(monkeypatch,
                      _plain_call(cl(x.cuda()), cl(w.cuda()), stride, pad))
    assert bool((got != 0).any())
    assert torch.equal(got, want)
    if fp64:
        _assert_fp64(got, x, w, stride, pad, BF16, "plain %s" % (x_shape,))


def test_plain_tile_fp16(monkeypatch):
    x_shape, w_shape = (2, 65, 10, 10), (65, 65, 5, 5)
    x, w = _plain_inputs(x_shape, w_shape, FP16, 8)
    got, want = _both(monkeypatch,
                      _plain_call(cl(x.cuda()), cl(w.cuda()), 1, 4))
    assert torch.equal(got, want)
    _assert_fp64(got, x, w, 1, 4, FP16, "plain fp16")


# noisy tile edges: K and MI at and past the 8 x 7 fragment limits
NOISY_CASES = [
    ((2, 16, 14, 14), (128, 16, 5, 5), 1, 0, "7x8"),
    ((2, 16, 14, 14), (129, 16, 5, 5), 1, 0, "generic"),
    ((2, 16, 12, 12), (65, 16, 3, 3), 1, 0, "7x5"),     # MI = 100, 5 N-frags
    ((2, 16, 8, 12), (20, 16, 5, 3), 1, 1, "5x2"),      # 5x3 filter, MI = 72
    ((1, 16, 10, 16), (20, 16, 3, 3), 1, 0, "7x2"),     # MI = 112 exactly
    ((1, 13, 11, 11), (70, 13, 3, 3), 1, 1, "generic"),  # MI = 121 > 112
    ((3, 24, 15, 15), (20, 24, 3, 3), 2, 1, "4x2"),     # stride 2, pad 1
]


@pytest.mark.parametrize("case", NOISY_CASES,
                         ids=lambda c: "x".join(map(str, c[0])) + "-k%d"
                         % c[1][0])
def test_noisy_tile_equals_generic(case, monkeypatch):
    x_shape, w_shape, stride, pad, tile = case
    inp = fo.make_inputs(x_shape, w_shape, BF16, seed=9)
    x, wq, w_raw = cl(inp.x.cuda()), cl(inp.wq.cuda()), cl(inp.w_raw.cuda())
    bias, factor = inp.bias.cuda(), torch.tensor([0.5], device='cuda')
    monkeypatch.setenv(ENV, "all")
    assert _tile(x_shape, w_shape, stride, pad, BF16, 2) == tile

    def call():
        return ops.ext().conv_fwd_fused(x, wq, w_raw, bias, stride, pad, 2,
                                        factor, SEED, False)[0]

    got, want = _both(monkeypatch, call, fitted="all")
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# one training step of the flagship model, default tiles vs the 64x64 tile
# ---------------------------------------------------------------------------

FLAGSHIP = ['--current', '1', '--q_a', '4', '--act_max', '5', '--batch_size',
            '64', '--calculate_running', '--no-augment']


def _one_step():
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(0, 16, (64, 3, 32, 32), generator=g).float() / 15.0)
    y = torch.randint(0, 10, (64,), generator=g).cuda()
    x = cl(x.cuda().bfloat16())
    args = build_noisynet_parser().parse_args(FLAGSHIP)
    broadcast_per_layer(args)
    torch.manual_seed(9)
    model = Net(args)
    utils.init_model(model, args)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.float()
    model = model.to(memory_format=torch.channels_last)
    start_calibration(model)
    with torch.no_grad():
        model(x, 0, 0)
    finish_calibration(model, torch.device('cuda'))
    model.train()
    torch.manual_seed(31)
    logits = model(x, 0, 100)
    ops.cross_entropy(logits, y).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    # the fused loss kernel sums with float atomics; compare a deterministic
    # loss of the same logits instead
    loss = F.cross_entropy(logits.detach().float(), y)
    return logits.detach().clone(), loss, grads


@pytest.mark.parametrize("fitted", [None, "all"], ids=["default", "all"])
def test_model_step_equals_generic(fitted, monkeypatch):
    (logits, loss, grads), (logits_g, loss_g, grads_g) = _both(
        monkeypatch, _one_step, fitted)
    assert torch.isfinite(loss)
    assert torch.equal(loss, loss_g)
    assert torch.equal(logits, logits_g)
    assert set(grads) == set(grads_g) and 'conv2.weight' in grads
    for n in grads:
        assert torch.equal(grads[n], grads_g[n]), n
