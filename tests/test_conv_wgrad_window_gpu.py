"""Window-staged patch wgrad (conv_wgrad_window_kernel, csrc/conv_mfma.hip).

The window kernel claims BIT-identity with conv_wgrad_patch_kernel, not a
tolerance: it writes the same [mslices, Kp, CRSp] f32 partials, and every
element is the same chain of 16x16x32 MFMAs (same m-slices, 128-m rounds in
ascending order, ks = 0..3, the same m in the same fragment position). So
each case runs ``conv_wgrad_patch`` on the default route and under
``NOISYNET_WGRAD_PATCH=legacy`` on the same inputs and compares with
``torch.equal``, and asserts what ``conv_wgrad_route`` reports. The first
four cases are also held to the bound of
``test_conv_wgrad_patch_matches_reference`` (max abs error / max |ref| < 0.02
against fp32 ``conv2d_weight``).

The noisy patch forward pads a 16-bit input with C % 8 != 0 to 8 channels
once and hands the copy to the weight gradient; that too is bit-identical
and is compared against ``NOISYNET_CONV_PAD_SHARE=0``.
"""

import pytest
import torch

from noisynet_amd import ops
from noisynet_amd.ops import functional as fn

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
ENV = "NOISYNET_WGRAD_PATCH"
WGRAD_BOUND = 0.02      # test_conv_wgrad_patch_matches_reference


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _route(case, dtype):
    N, C, H, W, K, R, stride, pad = case
    es = torch.empty(0, dtype=dtype).element_size()
    return ops.ext().conv_wgrad_route(C, H, W, K, R, R, stride, pad, es)


def _inputs(case, dtype, seed):
    N, C, H, W, K, R, stride, pad = case
    g = torch.Generator().manual_seed(seed)
    OH = (H + 2 * pad - R) // stride + 1
    OW = (W + 2 * pad - R) // stride + 1
    x = (torch.randn((N, C, H, W), generator=g) * 0.5).to(dtype)
    gy = (torch.randn((N, K, OH, OW), generator=g) * 0.5).to(dtype)
    return x, gy


def _both(monkeypatch, case, dtype, seed=11):
    """conv_wgrad_patch under the default route, then under the legacy one."""
    N, C, H, W, K, R, stride, pad = case
    x, gy = _inputs(case, dtype, seed)
    xg, gg = cl(x.cuda()), cl(gy.cuda())

    def call():
        return ops.ext().conv_wgrad_patch(gg, xg, stride, pad, R, R)

    monkeypatch.delenv(ENV, raising=False)
    got = call()
    monkeypatch.setenv(ENV, "legacy")
    assert _route(case, dtype) == "legacy"
    want = call()
    monkeypatch.delenv(ENV, raising=False)
    assert got.shape == (K, C, R, R)
    assert bool((got != 0).any())
    return x, gy, got, want


def _assert_reference(case, x, gy, got):
    N, C, H, W, K, R, stride, pad = case
    ref = torch.nn.grad.conv2d_weight(x.float(), (K, C, R, R), gy.float(),
                                      stride, pad)
    err = (got.float().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print("%s: err/scale = %.3g" % (case, err / scale))
    assert err / scale < WGRAD_BOUND, (case, err / scale)


# (N, C, H, W, K, R, stride, pad)
CONV2 = (5, 65, 14, 14, 120, 5, 1, 0)
WINDOW_CASES = [
    # M = 500: rounds straddle image boundaries, the last round is partial,
    # C padded 65 -> 72, K < 128
    CONV2,
    # chunks = 2 (141 rounds over 71 slices), slice edges not on image edges
    (180, 65, 14, 14, 120, 5, 1, 0),
    # padded conv, narrow K: taps in the zero border, one active column group
    (4, 24, 16, 16, 32, 3, 1, 1),
    # K > 128: two k-tiles, the second 8 wide
    (2, 16, 8, 8, 136, 3, 1, 1),
]


@pytest.mark.parametrize("case", WINDOW_CASES,
                         ids=lambda c: "x".join(map(str, c)))
def test_window_equals_legacy_and_reference(case, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    assert _route(case, BF16) == "window"
    x, gy, got, want = _both(monkeypatch, case, BF16)
    assert torch.equal(got, want)
    _assert_reference(case, x, gy, got)


def test_strided_takes_window_and_equals_legacy(monkeypatch):
    case = (4, 32, 16, 16, 64, 3, 2, 1)
    monkeypatch.delenv(ENV, raising=False)
    assert _route(case, BF16) == "window"
    _, _, got, want = _both(monkeypatch, case, BF16)
    assert torch.equal(got, want)


def test_fp16_equals_legacy(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    assert _route(CONV2, FP16) == "window"
    _, _, got, want = _both(monkeypatch, CONV2, FP16)
    assert got.dtype == FP16
    assert torch.equal(got, want)


def test_rejected_shape_reports_legacy_and_matches(monkeypatch):
    """9 output-row slots of 16 x 256 channels are 4608 16-byte chunks, more
    than the 4 per thread the window kernel stages; fp32 has no window
    kernel at all."""
    case = (2, 256, 16, 16, 32, 3, 1, 1)
    monkeypatch.delenv(ENV, raising=False)
    assert _route(case, BF16) == "legacy"
    assert _route(CONV2, torch.float32) == "legacy"
    x, gy, got, want = _both(monkeypatch, case, BF16)
    assert torch.equal(got, want)
    _assert_reference(case, x, gy, got)


def test_fused_noisy_conv_shared_padded_input(monkeypatch):
    """conv2's shape through _FusedNoisyConv: forward on the channel-padded
    copy and wgrad from that copy, against padding separately in each."""
    g = torch.Generator().manual_seed(17)
    x0 = (torch.rand((4, 65, 14, 14), generator=g) * 2).to(BF16)
    w0 = (torch.randn((120, 65, 5, 5), generator=g) * 0.1).to(BF16)
    gy = cl((torch.randn((4, 120, 10, 10), generator=g) * 0.5).to(BF16).cuda())
    seen = []
    real = ops.ext().conv_wgrad_patch

    def spy(*a, **k):
        seen.append(len(a) > 6 and a[6] is not None)
        return real(*a, **k)

    monkeypatch.setattr(ops.ext(), "conv_wgrad_patch", spy)

    def call():
        x = cl(x0.cuda()).requires_grad_(True)
        w = cl(w0.cuda()).requires_grad_(True)
        torch.manual_seed(23)
        y = fn.fused_noisy_conv2d(x, w, w.detach(), None, 1, 0, "abs2", 0.5)
        y.backward(gy)
        return y.detach(), x.grad, w.grad

    monkeypatch.delenv("NOISYNET_CONV_PAD_SHARE", raising=False)
    y, gx, gw = call()
    monkeypatch.setenv("NOISYNET_CONV_PAD_SHARE", "0")
    y0, gx0, gw0 = call()
    monkeypatch.delenv("NOISYNET_CONV_PAD_SHARE", raising=False)
    assert seen == [True, False]
    assert bool((y != 0).any()) and bool((gw != 0).any())
    assert torch.equal(y, y0)
    assert torch.equal(gx, gx0)
    assert torch.equal(gw, gw0)
