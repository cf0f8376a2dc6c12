"""The autograd routing layer above the conv kernels, against torch in fp64.

ops.conv2d / ops.fused_noisy_conv2d choose a dgrad and a wgrad kernel per
shape (_conv_dgrad_raw, _conv_wgrad_raw). One case per branch: .backward()
with a representable upstream gradient, the gradients of x, w and bias
compared with fp64 autograd under the oracle's deterministic bound, and the
extension entry points that ran recorded, so that a case cannot silently
test another branch than the one it names.
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32

ROUTED = ("conv_fwd", "conv_fwd_fused", "conv_dgrad", "linear_dgrad",
          "conv_wgrad", "conv_wgrad_from_col", "conv_wgrad_patch",
          "conv_wgrad_im2col", "linear_wgrad")


@pytest.fixture
def calls(monkeypatch):
    """Names of the routed extension entry points, in call order."""
    mod = ops.ext()
    seen = []

    def spy(name):
        real = getattr(mod, name)

        def wrapper(*a, **k):
            seen.append(name)
            return real(*a, **k)
        return wrapper

    for name in ROUTED:
        monkeypatch.setattr(mod, name, spy(name))
    return seen


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def to_kcrs(t):
    return t.detach().cpu().double()


def assert_within(got, ref, bound, what):
    # gradients keep their own layout: compare element by element
    err = (got - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err),
                              err / bound.clamp_min(1e-300)).max())
    print("%s: worst |err|/bound = %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: |err| reaches %.3g x the derived bound" % (
        what, ratio)


# id, api, dtype, (N, C, H, W, K, R, stride, pad), dgrad entry, wgrad entry
# ("patch" dgrad = conv_fwd_fused on the flipped filter, called from backward)
CASES = [
    ("patch_dgrad_5x5", "conv2d", BF16, (2, 13, 12, 12, 20, 5, 1, 0),
     "conv_fwd_fused", "conv_wgrad_patch"),
    ("patch_dgrad_3x3_pad1", "conv2d", FP16, (3, 13, 11, 11, 70, 3, 1, 1),
     "conv_fwd_fused", "conv_wgrad_patch"),
    ("pointwise", "conv2d", BF16, (2, 40, 7, 7, 70, 1, 1, 0),
     "linear_dgrad", "linear_wgrad"),
    ("dgrad_stride2", "conv2d", BF16, (2, 24, 15, 15, 20, 3, 2, 1),
     "conv_dgrad", "conv_wgrad_patch"),
    ("dgrad_k8", "conv2d", BF16, (2, 13, 10, 10, 8, 3, 1, 1),
     "conv_dgrad", "conv_wgrad_patch"),
    ("wgrad_from_col", "fused", BF16, (3, 3, 15, 15, 65, 5, 1, 0),
     "conv_fwd_fused", "conv_wgrad_from_col"),
    ("wgrad_from_col_c8", "fused", FP16, (2, 8, 9, 9, 20, 2, 1, 0),
     "conv_fwd_fused", "conv_wgrad_from_col"),
    ("wgrad_im2col_fp32", "conv2d", FP32, (2, 13, 11, 11, 20, 3, 1, 1),
     "conv_fwd_fused", "conv_wgrad_im2col"),
    ("wgrad_downsample", "conv2d", BF16, (2, 32, 14, 14, 64, 1, 2, 0),
     "conv_dgrad", "conv_wgrad"),
    ("wgrad_downsample_fp32", "conv2d", FP32, (2, 32, 14, 14, 64, 1, 2, 0),
     "conv_dgrad", "conv_wgrad"),
    # the same shapes through the other public entry point
    ("fused_patch", "fused", BF16, (3, 13, 11, 11, 70, 3, 1, 1),
     "conv_fwd_fused", "conv_wgrad_patch"),
    ("fused_stream_stride2", "fused", BF16, (1, 16, 56, 56, 24, 3, 2, 1),
     "conv_dgrad", "conv_wgrad_patch"),
]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_backward_matches_fp64(case, bias, calls):
    name, api, dtype, shape, dgrad_fn, wgrad_fn = case
    N, C, H, W, K, R, stride, pad = shape
    inp = fo.make_inputs((N, C, H, W), (K, C, R, R), dtype, seed=3)
    OH = (H + 2 * pad - R) // stride + 1
    gen = torch.Generator().manual_seed(4)
    gy = torch.randn(N, K, OH, OH, generator=gen).to(dtype)

    x = cl(inp.x.cuda()).requires_grad_()
    w = cl(inp.wq.cuda()).requires_grad_()
    b = inp.bias.cuda().requires_grad_() if bias else None
    if api == "conv2d":
        y = ops.conv2d(x, w, b, stride, pad)
    else:
        y = ops.fused_noisy_conv2d(x, w, cl(inp.w_raw.cuda()), b, stride, pad,
                                   "abs", 0.0)
    del calls[:]
    y.backward(cl(gy.cuda()))
    print(name, "backward ran", calls)
    assert dgrad_fn in calls and wgrad_fn in calls
    assert len(calls) == 2

    x64, w64, g64 = inp.x.double(), inp.wq.double(), gy.double()
    gx_ref = torch.nn.grad.conv2d_input(x64.shape, w64, g64, stride, pad)
    gx_A = torch.nn.grad.conv2d_input(x64.shape, w64.abs(), g64.abs(), stride,
                                      pad)
    gw_ref = torch.nn.grad.conv2d_weight(x64, w64.shape, g64, stride, pad)
    gw_A = torch.nn.grad.conv2d_weight(x64.abs(), w64.shape, g64.abs(),
                                       stride, pad)
    M = N * OH * OH
    # dgrad contracts over K*R*R (plus a partial sum per tap); wgrad over M,
    # in slices of at least one 32-deep chunk whose fp32 partials are added
    n_dgrad = K * R * R + R * R
    n_wgrad = M + -(-M // 32)
    assert_within(to_kcrs(x.grad), gx_ref,
                     fo.det_bound(gx_ref, gx_A, n_dgrad, dtype), name + " dx")
    assert_within(to_kcrs(w.grad), gw_ref,
                     fo.det_bound(gw_ref, gw_A, n_wgrad, dtype), name + " dw")
    if bias:
        gb_ref = g64.sum(dim=(0, 2, 3))
        gb_A = g64.abs().sum(dim=(0, 2, 3))
        assert_within(to_kcrs(b.grad), gb_ref,
                         fo.det_bound(gb_ref, gb_A, M, dtype), name + " db")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype,shape", [(BF16, (200, 96, 65)),
                                         (FP16, (70, 390, 10)),
                                         (FP32, (130, 200, 100))])
def test_linear_backward_matches_fp64(dtype, shape, bias):
    M, Kc, K = shape
    inp = fo.make_inputs((M, Kc), (K, Kc), dtype, seed=5)
    gen = torch.Generator().manual_seed(6)
    gy = torch.randn(M, K, generator=gen).to(dtype)
    x = inp.x.cuda().requires_grad_()
    w = inp.wq.cuda().requires_grad_()
    b = inp.bias.cuda().requires_grad_() if bias else None
    y = ops.fused_noisy_linear(x, w, inp.w_raw.cuda(), b, "abs2", 0.0)
    y.backward(gy.cuda())
    x64, w64, g64 = inp.x.double(), inp.wq.double(), gy.double()
    what = "linear %s " % (shape,)
    assert_within(to_kcrs(x.grad), g64 @ w64,
                  fo.det_bound(g64 @ w64, g64.abs() @ w64.abs(), K, dtype),
                  what + "dx")
    assert_within(to_kcrs(w.grad), g64.t() @ x64,
                  fo.det_bound(g64.t() @ x64, g64.abs().t() @ x64.abs(),
                               M + -(-M // 32), dtype), what + "dw")
    if bias:
        assert_within(to_kcrs(b.grad), g64.sum(0),
                      fo.det_bound(g64.sum(0), g64.abs().sum(0), M, dtype),
                      what + "db")


# ---------------------------------------------------------------------------
# double backward (the gradient penalties differentiate dgrad again)
# ---------------------------------------------------------------------------

# max error over max |ref|: twice the loosest per-kernel fp32 bound the suite
# asserts (1e-4 for wgrad in test_conv_exact_dtype_paths); the chain runs two
# kernels deep. Measured on MI355X: 6.0e-7 at worst (patch route, dx).
DOUBLE_BACKWARD_REL = 2e-4


def _penalty(conv, x, w, stride, pad):
    y = conv(x, w, None, stride, pad)
    gx = torch.autograd.grad(y.square().sum(), x, create_graph=True)[0]
    return gx.square().sum()


@pytest.mark.parametrize("name,shape,fwd", [
    ("patch", (2, 13, 11, 11, 20, 3, 1, 1), "conv_fwd_fused"),
    ("stream", (2, 8, 10, 10, 12, 3, 1, 1), "conv_fwd"),
])
def test_double_backward_fp32(name, shape, fwd, calls):
    N, C, H, W, K, R, stride, pad = shape
    inp = fo.make_inputs((N, C, H, W), (K, C, R, R), FP32, seed=7)
    x = cl(inp.x.cuda()).requires_grad_()
    w = cl(inp.wq.cuda()).requires_grad_()
    p = _penalty(ops.conv2d, x, w, stride, pad)
    assert calls[0] == fwd
    p.backward()
    print(name, "ran", calls)
    x64 = inp.x.double().requires_grad_()
    w64 = inp.wq.double().requires_grad_()
    p64 = _penalty(F.conv2d, x64, w64, stride, pad)
    p64.backward()
    for what, got, ref in (("dx", x.grad, x64.grad), ("dw", w.grad, w64.grad),
                           ("p", p, p64)):
        ref = ref.detach()
        rel = float((to_kcrs(got) - ref).abs().max() / ref.abs().max())
        print("double backward %s %s: max err / max |ref| = %.3g" % (
            name, what, rel))
        assert rel <= DOUBLE_BACKWARD_REL
