"""Differential crossbar columns on the CPU: the fp64 oracle itself, the
pure-PyTorch op (``differential=True``) against it, the flag and the model
wiring."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_diff_oracle as xd  # noqa: E402
import xbar_oracle as xo  # noqa: E402
from noisynet_amd import ops  # noqa: E402
from noisynet_amd.config import (broadcast_per_layer,  # noqa: E402
                                 build_noisynet_parser)
from noisynet_amd.models.noisynet import Net  # noqa: E402

CONV_A = ((3, 5, 9, 9), (70, 5, 5, 5), 2, 2)       # odd C, n = 125, padding
LINEAR = ((130, 296), (80, 296))
EXACT_CFGS = [(128, 5, 248.0), (64, 5, 124.0), (32, 6, 63.0)]  # steps 8, 4, 1


def _conv_inputs(dtype=torch.float32, seed=1):
    xs, ws, stride, pad = CONV_A
    return fo.make_inputs(xs, ws, dtype, seed), stride, pad


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def test_oracle_columns_subtract_to_the_plain_op():
    inp, stride, pad = _conv_inputs()
    ref = xd.conv_blocked(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad,
                          "abs2", 32, 0, 0.0)
    want = fo.to_mk(F.conv2d(inp.x.double(), inp.wq.double(),
                             inp.bias.double(), stride, pad))
    assert ref.nblocks == 4 and len(ref.t) == 8 and len(ref.s) == 8
    assert ref.n_partials == 8 * ref.out.numel()
    assert float((ref.out - want).abs().max()) <= 1e-12
    assert float((ref.clean - want).abs().max()) <= 1e-12
    # the two columns' sigmas add up to the existing oracle's block sigma
    # (here all x >= 0), and their |x| wq sums to its A
    old = xo.conv_blocked(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad,
                          "abs2", 32, 0, 0.0)
    assert float(inp.x.min()) >= 0
    for b in range(4):
        assert float((ref.s[2 * b] + ref.s[2 * b + 1] - old.s[b]).abs().max()) \
            <= 1e-12
        assert float((ref.A[2 * b] + ref.A[2 * b + 1] - old.A[b]).abs().max()) \
            <= 1e-12
        assert float((ref.s_abs[b] - old.s_abs[b]).abs().max()) == 0.0


def test_oracle_unipolar_rounding_and_clipping():
    x = torch.tensor([[1.0, 1.0]])
    w = torch.tensor([[0.5, 0.0], [1.5, 0.0], [2.5, 0.0], [100.0, 0.0],
                      [-100.0, 0.0], [3.0, -1.5]])
    # bits 3 -> Qu 7, adc_max 7 -> step 1
    ref = xd.linear_blocked(x, w, None, None, None, 32, 3, 7.0)
    assert ref.step == 1.0 and ref.qu == 7.0
    assert ref.out.tolist() == [[0.0, 2.0, 2.0, 7.0, -7.0, 1.0]]
    assert ref.clipped == 2 and ref.absmax == 100.0
    # a negative input drives a column below zero: clamped to 0 and counted
    ref = xd.linear_blocked(-x, w, None, None, None, 32, 3, 7.0)
    assert ref.out.tolist() == [[0.0] * 6]
    assert ref.clipped == 6     # -0.5 rounds to -0.0, which is not below zero


def test_oracle_signed_range_clips_most_column_partials():
    # the figure that motivates the mode: a range sized for the signed block
    # partial, here the 56.0 that test_xbar_gpu.py uses for 64-row blocks,
    # clips most column partials. A full column sums 64 products of mean
    # 7.5 * (1 + ... + 8) / (8 * 17) = 1.99, i.e. about 127 >> 56.
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, 16, (130, 296), generator=gen).float()
    w = torch.randint(-8, 9, (80, 296), generator=gen).float() / 8
    old = xo.linear_blocked(x, w, None, None, None, 64, 4, 56.0)
    ref = xd.linear_blocked(x, w, None, None, None, 64, 4, 56.0)
    assert old.clipped / float(old.nblocks * old.out.numel()) < 0.5
    assert xd.clip_share(ref) > 0.5


# ---------------------------------------------------------------------------
# the pure-PyTorch op against the oracle
# ---------------------------------------------------------------------------


def test_cpu_exact_case_is_bit_equal():
    # integer-grid inputs and a power-of-two step: exact in fp32 and fp64
    gen = torch.Generator().manual_seed(4)
    x = torch.randint(0, 16, (130, 296), generator=gen).float()
    w = torch.randint(-8, 9, (80, 296), generator=gen).float() / 8
    b = torch.randint(-8, 9, (80,), generator=gen).float() / 8
    for rows, bits, amax in EXACT_CFGS:
        ref = xd.linear_blocked(x, w, None, b, None, rows, bits, amax)
        t = ops.XbarTelemetry()
        out = ops.xbar_noisy_linear(x, w, w, b, None, 0.0, rows, bits, amax,
                                    want_telemetry=True, telemetry_out=t,
                                    differential=True)
        assert torch.equal(out.double(), ref.out)
        assert xd.clip_share(ref) > 0.01 and xd.tie_share(ref) > 0.002
        assert float(t.partial_absmax) == ref.absmax
        assert abs(float(t.adc_clip_share) - xd.clip_share(ref)) <= 1e-6
    xs, ws, stride, pad = CONV_A
    xc = torch.randint(0, 16, xs, generator=gen).float()
    wc = torch.randint(-8, 9, ws, generator=gen).float() / 8
    bc = torch.randint(-8, 9, (ws[0],), generator=gen).float() / 8
    for rows, bits, amax in EXACT_CFGS:
        ref = xd.conv_blocked(xc, wc, None, bc, stride, pad, None, rows, bits,
                              amax)
        out = ops.xbar_noisy_conv2d(xc, wc, wc, bc, stride, pad, None, 0.0,
                                    rows, bits, amax, differential=True)
        assert out.shape == (3, 70, 5, 5)
        assert torch.equal(fo.to_mk(out).double(), ref.out)


@pytest.mark.parametrize("cfg", [(64, 5, 3.0), (32, 4, 1.5)])
def test_cpu_conv_matches_oracle(cfg):
    rows, bits, amax = cfg
    inp, stride, pad = _conv_inputs()
    ref = xd.conv_blocked(inp.x, inp.wq, None, inp.bias, stride, pad, None,
                          rows, bits, amax)
    t = ops.XbarTelemetry()
    out = ops.xbar_noisy_conv2d(inp.x, inp.wq, inp.w_raw, inp.bias, stride,
                                pad, None, 0.0, rows, bits, amax,
                                want_telemetry=True, telemetry_out=t,
                                differential=True)
    assert out.shape == (3, 70, 5, 5) and out.dtype == torch.float32
    xd.assert_adc_close(out, ref, rows, torch.float32,
                        "cpu diff conv %s" % (cfg,))
    assert abs(float(t.partial_absmax) - ref.absmax) <= 1e-5 * ref.absmax
    assert abs(float(t.adc_clip_share) - xd.clip_share(ref)) <= 0.01
    assert t.power is None and t.nsr is None


@pytest.mark.parametrize("cfg", [(128, 6, 6.0), (64, 4, 3.0), (32, 7, 1.5)])
def test_cpu_linear_matches_oracle(cfg):
    rows, bits, amax = cfg
    inp = fo.make_inputs(*LINEAR, torch.float32, 1)
    for bias in (inp.bias, None):
        ref = xd.linear_blocked(inp.x, inp.wq, None, bias, None, rows, bits,
                                amax)
        out = ops.xbar_noisy_linear(inp.x, inp.wq, inp.w_raw, bias, None, 0.0,
                                    rows, bits, amax, differential=True)
        xd.assert_adc_close(out, ref, rows, torch.float32,
                            "cpu diff linear %s" % (cfg,))


def test_cpu_noise_with_adc_off_is_the_unblocked_model():
    # for x >= 0 the column sigmas add up to the block's: variance
    # factor * sum_b s_b, exactly the existing model's
    inp = fo.make_inputs((1700, 296), (80, 296), torch.float32, 5)
    assert float(inp.x.min()) >= 0
    refs = fo.linear_refs(inp.x, inp.wq, inp.w_raw, inp.bias, "abs")
    torch.manual_seed(11)
    out = ops.xbar_noisy_linear(inp.x, inp.wq, inp.w_raw, inp.bias, "abs",
                                0.5, 64, 0, 0.0, differential=True)
    fo.check_noise_field(out, refs.clean, refs.sig, 0.5,
                         stats=("mean", "std", "kurtosis", "channel_std"),
                         what="cpu differential noise")


def test_cpu_column_draws_are_independent():
    # w = [wb, -wb] over x = [xb, xb]: the clean output is zero and the two
    # columns carry the same sigma; a shared draw would cancel to zero noise
    gen = torch.Generator().manual_seed(9)
    xb = torch.randint(1, 16, (2000, 32), generator=gen).float() / 15
    wb = torch.randn(80, 32, generator=gen) * 0.05
    x, w = xb.repeat(1, 2), torch.cat([wb, -wb], 1)
    ref = xd.linear_blocked(x, w, w, None, "abs", 64, 0, 0.0)
    assert ref.nblocks == 1
    assert float(ref.clean.abs().max()) <= 1e-12
    assert float((ref.s[0] - ref.s[1]).abs().max()) <= 1e-12
    torch.manual_seed(12)
    out = ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 0, 0.0,
                                differential=True)
    fo.check_noise_field(out, ref.clean, 2 * ref.s[0], 0.5,
                         stats=("mean", "std", "channel_std"),
                         what="cpu two columns")
    assert float((out != 0).double().mean()) > 0.5


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
        x, w, inp.w_raw, b, stride, pad, "abs", 0.5, 32, 4, 1.0,
        differential=True))
    same = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    for a, s in zip(got, same):
        assert torch.equal(a, s)

    lin = fo.make_inputs(*LINEAR, torch.float32, 7)
    gl = torch.randn(130, 80, generator=torch.Generator().manual_seed(8))

    def lgrads(fn):
        x = lin.x.clone().requires_grad_()
        w = lin.wq.clone().requires_grad_()
        b = lin.bias.clone().requires_grad_()
        fn(x, w, b).backward(gl)
        return x.grad, w.grad, b.grad

    got = lgrads(lambda x, w, b: ops.xbar_noisy_linear(
        x, w, lin.w_raw, b, None, 0.0, 64, 4, 2.0, differential=True))
    same = lgrads(lambda x, w, b: ops.linear(x, w, b))
    for a, s in zip(got, same):
        assert torch.equal(a, s)


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
                              kw["xbar_rows"], kw["adc_bits"], kw["adc_max"],
                              differential=True)
    xc, wc = torch.rand(1, 4, 6, 6), torch.randn(8, 4, 3, 3)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_conv2d(xc, wc, wc, None, 1, 0, kw["sigma_mode"], 0.5,
                              kw["xbar_rows"], kw["adc_bits"], kw["adc_max"],
                              differential=True)


def test_unipolar_adc_params():
    adc = ops.reference.xbar_adc_params(5, 248.0, "cpu", unipolar=True)
    assert adc.tolist() == [8.0, 0.125]
    adc = ops.reference.xbar_adc_params(5, 248.0, "cpu")
    assert adc[0].item() == pytest.approx(248.0 / 15)
    assert ops.reference.xbar_adc_params(0, 0.0, "cpu", unipolar=True) is None


# ---------------------------------------------------------------------------
# flag and model
# ---------------------------------------------------------------------------


def _args(extra=()):
    argv = ['--n_train', '64', '--n_test', '32', '--batch_size', '8',
            '--nepochs', '1'] + list(extra)
    return broadcast_per_layer(build_noisynet_parser().parse_args(argv))


def test_flag_parses():
    assert _args().xbar_diff is False
    assert _args(['--xbar_rows', '64', '--xbar_diff']).xbar_diff is True


def test_xbar_diff_without_xbar_rows_raises():
    with pytest.raises(ValueError, match=r"xbar_diff.*xbar_rows"):
        Net(_args(['--xbar_diff']))
    with pytest.raises(ValueError, match=r"xbar_diff.*xbar_rows"):
        Net(_args(['--xbar_diff', '--xbar_rows', '0', '--current', '1']))


def test_model_xbar_diff_step_on_cpu(monkeypatch):
    seen = []
    conv, lin = ops.xbar_noisy_conv2d, ops.xbar_noisy_linear

    def spy_conv(*a, **k):
        seen.append(k.get("differential"))
        return conv(*a, **k)

    def spy_lin(*a, **k):
        seen.append(k.get("differential"))
        return lin(*a, **k)

    monkeypatch.setattr(ops, "xbar_noisy_conv2d", spy_conv)
    monkeypatch.setattr(ops, "xbar_noisy_linear", spy_lin)
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
               '--xbar_diff', '--q_adc', '6', '--adc_max', '6'])
    torch.manual_seed(0)
    m = Net(a)
    m.train()
    x = torch.rand(8, 3, 32, 32)
    y = torch.randint(0, 10, (8,))
    loss = F.cross_entropy(m(x, 0, 0), y)
    loss.backward()
    assert torch.isfinite(loss)
    assert seen == [True] * 4
    for name in ('conv1', 'conv2', 'linear1', 'linear2'):
        g = getattr(m, name).weight.grad
        assert g is not None and torch.isfinite(g).all(), name
    for k in range(4):
        assert len(m.adc_clip[k]) == 1 and 0.0 <= m.adc_clip[k][0] <= 1.0
        assert m.partial_absmax[k][0] > 0
        assert len(m.power[k]) == 1 and len(m.nsr[k]) == 1


def test_model_without_the_flag_passes_differential_off(monkeypatch):
    seen = []
    conv, lin = ops.xbar_noisy_conv2d, ops.xbar_noisy_linear

    def spy_conv(*a, **k):
        seen.append(k.get("differential"))
        return conv(*a, **k)

    def spy_lin(*a, **k):
        seen.append(k.get("differential"))
        return lin(*a, **k)

    monkeypatch.setattr(ops, "xbar_noisy_conv2d", spy_conv)
    monkeypatch.setattr(ops, "xbar_noisy_linear", spy_lin)
    a = _args(['--xbar_rows', '64', '--q_adc', '5', '--adc_max', '2'])
    m = Net(a)
    out = m(torch.rand(8, 3, 32, 32), 0, 0)
    assert torch.isfinite(out).all()
    assert seen == [False] * 4


def test_print_xbar_stats_names_the_mode(capsys):
    from noisynet_amd.drivers.cifar import print_xbar_stats
    a = _args(['--xbar_rows', '64', '--xbar_diff', '--q_adc', '5',
               '--adc_max', '4'])
    m = Net(a)
    m(torch.rand(8, 3, 32, 32), 0, 0)
    print_xbar_stats(m, a)
    text = capsys.readouterr().out
    assert "differential columns, unipolar ADC" in text
    assert "per column" in text
