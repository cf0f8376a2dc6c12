"""Tiled crossbars on the CPU: the fp64 oracle itself, the pure-PyTorch op
against it, the flags and the model wiring."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_oracle as xo  # noqa: E402
from noisynet_amd import ops  # noqa: E402
from noisynet_amd.config import (broadcast_per_layer,  # noqa: E402
                                 build_noisynet_parser)
from noisynet_amd.models.noisynet import Net  # noqa: E402

CONV_A = ((3, 5, 9, 9), (70, 5, 5, 5), 2, 2)       # odd C, n = 125, padding
LINEAR = ((130, 296), (80, 296))


def _conv_inputs(dtype=torch.float32, seed=1):
    xs, ws, stride, pad = CONV_A
    return fo.make_inputs(xs, ws, dtype, seed), stride, pad


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def test_oracle_one_block_no_adc_is_the_plain_op():
    inp, stride, pad = _conv_inputs()
    ref = xo.conv_blocked(inp.x, inp.wq, None, inp.bias, stride, pad, None,
                          1024, 0, 0.0)
    want = fo.to_mk(F.conv2d(inp.x.double(), inp.wq.double(),
                             inp.bias.double(), stride, pad))
    assert ref.nblocks == 1
    assert float((ref.out - want).abs().max()) <= 1e-12
    lin = fo.make_inputs(*LINEAR, torch.float32, 2)
    ref = xo.linear_blocked(lin.x, lin.wq, None, lin.bias, None, 1024, 0, 0.0)
    want = F.linear(lin.x.double(), lin.wq.double(), lin.bias.double())
    assert float((ref.out - want).abs().max()) <= 1e-12


def test_oracle_blocks_without_adc_sum_to_the_plain_op():
    inp, stride, pad = _conv_inputs()
    ref = xo.conv_blocked(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad,
                          "abs2", 32, 0, 0.0)
    assert ref.nblocks == 4 and ref.n == 125
    assert float((ref.out - ref.clean).abs().max()) <= 1e-12
    # the block sigmas add up to the unblocked sigma (here all x >= 0)
    refs = fo.conv_refs(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad, "abs2")
    assert float((sum(ref.s) - refs.sig).abs().max()) <= 1e-12
    assert float((sum(ref.A) + ref.bias_abs - refs.A).abs().max()) <= 1e-12


def test_oracle_row_order_matters():
    # blocks cut the (r,s,c) order; cutting (c,r,s) instead must change the
    # quantised result, or the oracle could not catch a layout mix-up
    inp, stride, pad = _conv_inputs()
    a = xo.conv_blocked(inp.x, inp.wq, None, None, stride, pad, None, 32, 4,
                        1.0)
    b = xo.conv_blocked(inp.x, inp.wq, None, None, stride, pad, None, 32, 4,
                        1.0, order="crs")
    assert float((a.clean - b.clean).abs().max()) <= 1e-12   # same conv
    differ = float(((a.out - b.out).abs() > 0.5 * a.step).double().mean())
    print("outputs that differ between the row orders: %.3f" % differ)
    assert differ > 0.2


def test_oracle_rounds_half_to_even_and_clips():
    x = torch.tensor([[1.0, 1.0]])
    w = torch.tensor([[0.5, 0.0], [1.5, 0.0], [2.5, 0.0], [100.0, 0.0],
                      [-100.0, 0.0]])
    # bits 4 -> Qm 7, adc_max 7 -> step 1: t = 0.5, 1.5, 2.5, 100, -100
    ref = xo.linear_blocked(x, w, None, None, None, 32, 4, 7.0)
    assert ref.step == 1.0 and ref.qm == 7.0
    assert ref.out.tolist() == [[0.0, 2.0, 2.0, 7.0, -7.0]]
    assert ref.clipped == 2 and ref.absmax == 100.0


# ---------------------------------------------------------------------------
# the pure-PyTorch op against the oracle
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cfg", [(64, 5, 1.5), (32, 4, 1.0), (128, 6, 3.0)])
def test_cpu_conv_matches_oracle(cfg):
    rows, bits, amax = cfg
    inp, stride, pad = _conv_inputs()
    ref = xo.conv_blocked(inp.x, inp.wq, None, inp.bias, stride, pad, None,
                          rows, bits, amax)
    t = ops.XbarTelemetry()
    out = ops.xbar_noisy_conv2d(inp.x, inp.wq, inp.w_raw, inp.bias, stride,
                                pad, None, 0.0, rows, bits, amax,
                                want_telemetry=True, telemetry_out=t)
    assert out.shape == (3, 70, 5, 5) and out.dtype == torch.float32
    xo.assert_adc_close(out, ref, rows, torch.float32, "cpu conv %s" % (cfg,))
    assert abs(float(t.partial_absmax) - ref.absmax) <= 1e-5 * ref.absmax
    share = ref.clipped / float(ref.nblocks * ref.out.numel())
    assert abs(float(t.adc_clip_share) - share) <= 0.01
    assert t.power is None and t.nsr is None


@pytest.mark.parametrize("cfg", [(128, 6, 3.0), (64, 4, 2.0), (32, 8, 1.5)])
def test_cpu_linear_matches_oracle(cfg):
    rows, bits, amax = cfg
    inp = fo.make_inputs(*LINEAR, torch.float32, 3)
    ref = xo.linear_blocked(inp.x, inp.wq, None, inp.bias, None, rows, bits,
                            amax)
    out = ops.xbar_noisy_linear(inp.x, inp.wq, inp.w_raw, inp.bias, None, 0.0,
                                rows, bits, amax)
    xo.assert_adc_close(out, ref, rows, torch.float32,
                        "cpu linear %s" % (cfg,))


def test_cpu_exact_case_is_bit_equal():
    # integer-grid inputs and a power-of-two step: exact in fp32 and fp64
    gen = torch.Generator().manual_seed(4)
    x = torch.randint(0, 16, (130, 296), generator=gen).float()
    w = torch.randint(-8, 9, (80, 296), generator=gen).float() / 8
    b = torch.randint(-8, 9, (80,), generator=gen).float() / 8
    for rows, bits, amax in ((128, 4, 112.0), (64, 4, 56.0), (32, 6, 62.0)):
        ref = xo.linear_blocked(x, w, None, b, None, rows, bits, amax)
        out = ops.xbar_noisy_linear(x, w, w, b, None, 0.0, rows, bits, amax)
        assert torch.equal(out.double(), ref.out)
        assert 0.01 < ref.clipped / float(ref.nblocks * ref.out.numel()) < 0.5


def test_cpu_noise_with_adc_off_is_the_unblocked_model():
    # block noises add up to variance factor * sum_b s_b
    inp = fo.make_inputs((1700, 296), (80, 296), torch.float32, 5)
    refs = fo.linear_refs(inp.x, inp.wq, inp.w_raw, inp.bias, "abs")
    torch.manual_seed(11)
    out = ops.xbar_noisy_linear(inp.x, inp.wq, inp.w_raw, inp.bias, "abs",
                                0.5, 64, 0, 0.0)
    fo.check_noise_field(out, refs.clean, refs.sig, 0.5,
                         stats=("mean", "std", "kurtosis", "channel_std"),
                         what="cpu blocked noise")


def test_cpu_gradients_are_those_of_the_plain_op():
    inp, stride, pad = _conv_inputs()
    g = torch.randn(3, 70, 5, 5, generator=torch.Generator().manual_seed(6))

    def grads(fn):
        x = inp.x.clone().requires_grad_()
        w = inp.wq.clone().requires_grad_()
        b = inp.bias.clone().requires_grad_()
        fn(x, w, b).backward(g)
        return x.grad, w.grad, b.grad

    got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
        x, w, inp.w_raw, b, stride, pad, "abs", 0.5, 32, 4, 1.0))
    same = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    want = grads(lambda x, w, b: F.conv2d(x, w, b, stride, pad))
    for a, s, w_ in zip(got, same, want):
        assert torch.equal(a, s)
        torch.testing.assert_close(a, w_, rtol=1e-5, atol=1e-5)

    lin = fo.make_inputs(*LINEAR, torch.float32, 7)
    gl = torch.randn(130, 80, generator=torch.Generator().manual_seed(8))

    def lgrads(fn):
        x = lin.x.clone().requires_grad_()
        w = lin.wq.clone().requires_grad_()
        b = lin.bias.clone().requires_grad_()
        fn(x, w, b).backward(gl)
        return x.grad, w.grad, b.grad

    got = lgrads(lambda x, w, b: ops.xbar_noisy_linear(
        x, w, lin.w_raw, b, None, 0.0, 64, 4, 2.0))
    same = lgrads(lambda x, w, b: ops.linear(x, w, b))
    want = lgrads(lambda x, w, b: F.linear(x, w, b))
    for a, s, w_ in zip(got, same, want):
        assert torch.equal(a, s)
        torch.testing.assert_close(a, w_, rtol=1e-5, atol=1e-5)


def test_cpu_double_backward_runs():
    inp, stride, pad = _conv_inputs()
    x = inp.x.clone().requires_grad_()
    w = inp.wq.clone().requires_grad_()
    y = ops.xbar_noisy_conv2d(x, w, inp.w_raw, None, stride, pad, "abs", 0.5,
                              32, 4, 1.0)
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    gx.square().sum().backward()
    assert w.grad is not None and torch.isfinite(w.grad).all()


@pytest.mark.parametrize("bad,match", [
    (dict(xbar_rows=48), "xbar_rows"),
    (dict(xbar_rows=0), "xbar_rows"),
    (dict(adc_bits=1), "adc_bits"),
    (dict(adc_bits=17), "adc_bits"),
    (dict(adc_bits=4, adc_max=0.0), "adc_max"),
    (dict(adc_bits=0, sigma_mode=None), "neither"),
    (dict(sigma_mode="abs3"), "sigma_mode"),
])
def test_argument_validation(bad, match):
    kw = dict(sigma_mode="abs", xbar_rows=64, adc_bits=4, adc_max=1.0)
    kw.update(bad)
    x, w = torch.rand(4, 96), torch.randn(8, 96)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_linear(x, w, w, None, kw["sigma_mode"], 0.5,
                              kw["xbar_rows"], kw["adc_bits"], kw["adc_max"])
    xc, wc = torch.rand(1, 4, 6, 6), torch.randn(8, 4, 3, 3)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_conv2d(xc, wc, wc, None, 1, 0, kw["sigma_mode"], 0.5,
                              kw["xbar_rows"], kw["adc_bits"], kw["adc_max"])


# ---------------------------------------------------------------------------
# flags and model
# ---------------------------------------------------------------------------


def _args(extra=()):
    argv = ['--n_train', '64', '--n_test', '32', '--batch_size', '8',
            '--nepochs', '1'] + list(extra)
    return broadcast_per_layer(build_noisynet_parser().parse_args(argv))


def test_flags_parse_and_broadcast():
    a = _args()
    assert a.xbar_rows == 0 and a.q_adc == 0 and a.adc_max == 0.0
    assert a.block_size is None and a.blocked is False   # untouched
    a = _args(['--xbar_rows', '128', '--q_adc', '6', '--adc_max', '3'])
    assert (a.xbar_rows, a.q_adc) == (128, 6)
    assert [a.adc_max1, a.adc_max2, a.adc_max3, a.adc_max4] == [3.0] * 4
    a = _args(['--xbar_rows', '64', '--q_adc', '4', '--adc_max1', '1',
               '--adc_max2', '2', '--adc_max3', '3', '--adc_max4', '4'])
    assert [a.adc_max1, a.adc_max2, a.adc_max3, a.adc_max4] == [1, 2, 3, 4]


def test_model_xbar_step_on_cpu():
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
               '--q_adc', '6', '--adc_max', '3'])
    torch.manual_seed(0)
    m = Net(a)
    m.train()
    x = torch.rand(8, 3, 32, 32)
    y = torch.randint(0, 10, (8,))
    loss = F.cross_entropy(m(x, 0, 0), y)
    loss.backward()
    assert torch.isfinite(loss)
    for name in ('conv1', 'conv2', 'linear1', 'linear2'):
        g = getattr(m, name).weight.grad
        assert g is not None and torch.isfinite(g).all(), name
    for k in range(4):
        assert len(m.adc_clip[k]) == 1 and 0.0 <= m.adc_clip[k][0] <= 1.0
        assert m.partial_absmax[k][0] > 0
        assert len(m.power[k]) == 1 and len(m.nsr[k]) == 1


def test_model_adc_only_layers():
    a = _args(['--xbar_rows', '64', '--q_adc', '5', '--adc_max', '2'])
    torch.manual_seed(0)
    m = Net(a)
    out = m(torch.rand(8, 3, 32, 32), 0, 0)
    assert torch.isfinite(out).all()
    assert all(len(m.adc_clip[k]) == 1 for k in range(4))
    assert all(len(m.power[k]) == 0 for k in range(4))


def test_model_without_xbar_rows_is_unchanged(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("xbar op reached with xbar_rows 0")

    monkeypatch.setattr(ops, "xbar_noisy_conv2d", boom)
    monkeypatch.setattr(ops, "xbar_noisy_linear", boom)
    outs = []
    for strip in (False, True):
        a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '0'])
        if strip:   # an args object from before the flags existed
            for name in ('xbar_rows', 'q_adc', 'adc_max', 'adc_max1',
                         'adc_max2', 'adc_max3', 'adc_max4'):
                delattr(a, name)
        torch.manual_seed(3)
        m = Net(a)
        m.train()
        x = torch.rand(8, 3, 32, 32)
        outs.append(m(x, 0, 0))
        assert len(m.power[0]) == 1 and not m.adc_clip[0]
    assert torch.equal(outs[0], outs[1])


def test_introspective_flags_refuse_xbar_rows():
    a = _args(['--plot', '--xbar_rows', '128', '--q_adc', '6', '--adc_max',
               '3'])
    with pytest.raises(ValueError, match=r"xbar_rows.*plot"):
        Net(a)
    a = _args(['--xbar_rows', '128', '--q_adc', '6', '--adc_max', '3'])
    m = Net(a)
    a.L3_act = 0.1          # set after construction: caught at the call
    with pytest.raises(ValueError, match=r"xbar_rows.*L3_act"):
        m(torch.rand(2, 3, 32, 32), 0, 0)


@pytest.mark.parametrize("extra,match", [
    (['--xbar_rows', '100'], "xbar_rows"),
    (['--xbar_rows', '64', '--q_adc', '1', '--adc_max', '1'], "q_adc"),
    (['--xbar_rows', '64', '--q_adc', '4'], "adc_max"),
])
def test_model_argument_validation(extra, match):
    with pytest.raises(ValueError, match=match):
        Net(_args(extra))
