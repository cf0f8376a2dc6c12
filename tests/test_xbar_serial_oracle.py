"""Bit-serial crossbar inputs on the CPU: the pure-PyTorch op against the fp64
oracle of xbar_serial_oracle.py, the code recovery the mode rests on, the
argument rules, the flag and the model wiring."""

import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_oracle as xo  # noqa: E402
import xbar_serial_oracle as xso  # noqa: E402
from noisynet_amd import ops  # noqa: E402
from noisynet_amd.config import (broadcast_per_layer,  # noqa: E402
                                 build_noisynet_parser)
from noisynet_amd.models.noisynet import Net  # noqa: E402
from noisynet_amd.ops import reference as ref_ops  # noqa: E402

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32


def _call(shape, inp, mode, factor, rows, bits, amax, bias=True, **kw):
    kind, xs, ws, stride, pad = xso.SHAPES[shape]
    b = inp.bias if bias else None
    if kind == "conv":
        return ops.xbar_noisy_conv2d(inp.x, inp.wq, inp.w_raw, b, stride, pad,
                                     mode, factor, rows, bits, amax, **kw)
    return ops.xbar_noisy_linear(inp.x, inp.wq, inp.w_raw, b, mode, factor,
                                 rows, bits, amax, **kw)


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def test_oracle_one_slice_is_the_unsliced_oracle():
    inp = xso.general_inputs("linear", FP32)
    a = xso.oracle("linear", FP32, "general", "abs2", 64, 5, 2.0, 4)
    b = xo.linear_blocked(inp.x, inp.wq, inp.w_raw, inp.bias, "abs2", 64, 5,
                          2.0)
    assert a.J == 1 and a.nblocks == b.nblocks == 5
    # code * fp32(1/15) against fp32(code/15): one fp32 rounding apart
    tol = 2.0 ** -22 * float(b.clean.abs().max() + sum(b.A).max())
    assert float((a.clean - b.clean).abs().max()) <= tol
    assert float((sum(a.s) - sum(b.s)).abs().max()) <= tol


def test_oracle_slices_without_adc_recombine():
    for D in (1, 2, 3, 4):
        r = xso.oracle("convA", FP32, "general", "abs", 32, 0, 0.0, D)
        assert r.J == -(-4 // D) and len(r.t) == r.J * r.nblocks
        assert float((r.out - r.clean).abs().max()) <= 1e-12
        one = xso.oracle("convA", FP32, "general", "abs", 32, 0, 0.0, 4)
        assert float((r.clean - one.clean).abs().max()) <= 1e-12
        # sigma_abs shift-adds to the unsliced one, the variance does not
        sa = sum(sh * s for sh, s in zip(r.shift, r.s_abs))
        assert float((sa - sum(one.s_abs)).abs().max()) <= 1e-12
        if D < 4:
            assert float((xso.noise_variance(r) - xso.noise_variance(one))
                         .min()) >= 0.0
            assert float(xso.noise_variance(r).sum()) \
                > 1.5 * float(xso.noise_variance(one).sum())


def test_oracle_top_slice_may_be_narrower():
    x = torch.tensor([[13.0, 0.0]])                 # 0b1101
    w = torch.tensor([[1.0, 0.0]])
    r = xso.linear_blocked(x, w, None, None, None, 32, 0, 0.0, 1.0, 4, 3)
    assert r.J == 2 and [float(t) for t in r.t] == [5.0, 1.0]
    assert r.shift == [1.0, 8.0] and float(r.out) == 13.0
    # negative and off-grid inputs are re-quantised, the top code saturates
    x = torch.tensor([[-3.0, 0.0], [2.4, 0.0], [99.0, 0.0]])
    r = xso.linear_blocked(x, w, None, None, None, 32, 0, 0.0, 1.0, 4, 1)
    assert r.out.flatten().tolist() == [0.0, 2.0, 15.0]


# ---------------------------------------------------------------------------
# the pure-PyTorch op against the oracle, noise off
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32],
                         ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", list(xso.GENERAL_CFGS))
def test_cpu_op_matches_oracle(shape, dtype):
    inp = xso.general_inputs(shape, dtype)
    for rows, bits, amax, D in xso.GENERAL_CFGS[shape]:
        r = xso.oracle(shape, dtype, "general", None, rows, bits, amax, D)
        t = ops.XbarTelemetry()
        out = _call(shape, inp, None, 0.0, rows, bits, amax, in_bits=4,
                    dac_bits=D, x_step=1.0 / 15.0, want_telemetry=True,
                    telemetry_out=t)
        assert out.dtype == dtype
        xso.assert_adc_close(out, r, rows, dtype, "cpu %s %s" % (
            shape, (rows, bits, amax, D)))
        assert abs(float(t.partial_absmax) - r.absmax) <= 1e-5 * r.absmax
        assert abs(float(t.adc_clip_share) - xso.clip_share(r)) <= 0.01
        assert t.power is None and t.nsr is None


def test_cpu_exact_case_is_bit_equal():
    for shape in xso.SHAPES:
        inp = xso.exact_inputs(shape, FP32)
        for rows, bits, amax, D in xso.EXACT_CFGS:
            r = xso.oracle(shape, FP32, "exact", None, rows, bits, amax, D)
            t = ops.XbarTelemetry()
            out = _call(shape, inp, None, 0.0, rows, bits, amax, in_bits=4,
                        dac_bits=D, x_step=1.0, want_telemetry=True,
                        telemetry_out=t)
            assert torch.equal(fo.to_mk(out), r.out)
            assert float(t.partial_absmax) == r.absmax
            share = xso.clip_share(r)
            assert abs(float(t.adc_clip_share) - share) <= 2.0 ** -22 * share


# ---------------------------------------------------------------------------
# the inputs chosen for the GPU tests stay inside their caps (oracle alone)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cfg", xso.EXACT_CFGS)
def test_exact_inputs_exercise_clipping_and_ties(cfg):
    r = xso.oracle("linear", FP32, "exact", None, *cfg)
    clip, ties = xso.clip_share(r), xso.tie_share(r)
    print("%s: clip share %.3f, tie share %.4f" % (cfg, clip, ties))
    assert clip > 0.01 and ties > 0.002, (clip, ties)


@pytest.mark.parametrize("dtype", [BF16, FP32],
                         ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", list(xso.GENERAL_CFGS))
def test_general_inputs_stay_inside_their_caps(shape, dtype):
    for cfg in xso.GENERAL_CFGS[shape]:
        r = xso.oracle(shape, dtype, "general", None, *cfg)
        excluded, worst = xso.adc_report(r.out, r, cfg[0], dtype)
        clip = xso.clip_share(r)
        print("%s %s: excluded %.4f, clip share %.4f" % (shape, cfg, excluded,
                                                        clip))
        assert worst == 0.0
        assert excluded <= 0.05 and clip > 0.005, (excluded, clip)


# ---------------------------------------------------------------------------
# code recovery: every code survives fake_quant_forward and the dtype
# ---------------------------------------------------------------------------

RANGES = [1.0, 5.0, 0.3, 6.25, math.e, 1e-3, 37.0]


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32],
                         ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("bits", range(1, 9))
def test_every_code_is_recovered(bits, dtype):
    ncodes = 2 ** bits
    D = -(-bits // 4)                       # the fewest bits per slice
    w = torch.zeros(1, 32, dtype=dtype)
    w[0, 0] = 1.0
    want = torch.arange(ncodes, dtype=torch.float64)
    for rng in RANGES:
        scale = max(rng / (ncodes - 1.0), 1e-6)
        mid = torch.arange(ncodes, dtype=torch.float32) * scale
        xq = ref_ops.fake_quant_forward(mid, bits, 0.0, rng, 0).to(dtype)
        x = torch.zeros(ncodes, 32, dtype=dtype)
        x[:, 0] = xq
        if dtype == BF16 and bits == 8:
            with pytest.raises(ValueError, match="in_bits"):
                ops.xbar_noisy_linear(x, w, w, None, "abs", 0.0, 32, 0, 0.0,
                                      in_bits=bits, dac_bits=D, x_step=scale)
            continue
        # the oracle's codes, and the op's through a unit weight (factor 0,
        # ADC off: out = x_step * code, recombined from the slices)
        code = xso.codes(x, scale, bits)[:, 0].double()
        assert int((code != want).sum()) == 0, (rng, "oracle codes")
        x32, w32 = x.float(), w.float()
        out = ops.xbar_noisy_linear(x32, w32, w32, None, "abs", 0.0, 32, 0,
                                    0.0, in_bits=bits, dac_bits=D,
                                    x_step=scale)
        got = torch.round(out[:, 0].double() / xso.dac_step(scale)[0])
        assert int((got != want).sum()) == 0, (rng, "op codes")


# ---------------------------------------------------------------------------
# recombination: the slices add up to sum code * x_step * wq
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_slices_recombine(shape, D):
    kind, xs, ws, stride, pad = xso.SHAPES[shape]
    inp = xso.general_inputs(shape, FP32)
    rows = 64
    out = _call(shape, inp, "abs", 0.0, rows, 0, 0.0, in_bits=4, dac_bits=D,
                x_step=1.0 / 15.0)
    if kind == "conv":
        refs = fo.conv_refs(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad,
                            "abs")
    else:
        refs = fo.linear_refs(inp.x, inp.wq, inp.w_raw, inp.bias, "abs")
    J, nblocks = -(-4 // D), -(-refs.n // rows)
    # contraction, the shift-add of J*nblocks partials, the x_step multiply
    # and fp32(code/15) against code * fp32(1/15)
    fo.assert_within(out, refs.clean,
                     fo.det_bound(refs.clean, refs.A, refs.n + J * nblocks + 2,
                                  FP32), "%s D=%d recombined" % (shape, D))


def test_cpu_slice_noise_variance():
    # codes in {0, 15}, D = 1, one block: four equal slices, independent
    # draws shift-added give variance 85 * factor * s_0 (225x if one draw
    # served every slice)
    gen = torch.Generator().manual_seed(9)
    M, K = 2000, 80
    x = torch.randint(0, 2, (M, 32), generator=gen).float()
    x[:, 0] = 1.0
    w = torch.randn(K, 32, generator=gen) * 0.05
    r = xso.linear_blocked(x, w, w, None, "abs", 32, 0, 0.0, 1.0 / 15, 4, 1)
    assert r.nblocks == 1 and r.J == 4
    assert float((r.s[0] - r.s[3]).abs().max()) == 0.0
    var = xso.noise_variance(r)
    assert float((var - 85.0 * r.s[0]).abs().max()) <= 1e-9
    torch.manual_seed(11)
    out = ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 32, 0, 0.0,
                                in_bits=4, dac_bits=1, x_step=1.0 / 15)
    fo.check_noise_field(out, r.clean, var, 0.5,
                         stats=("mean", "std", "channel_std"),
                         what="cpu four equal slices")


def test_cpu_gradients_are_those_of_the_plain_op():
    kind, xs, ws, stride, pad = xso.SHAPES["convA"]
    inp = xso.general_inputs("convA", FP32)
    g = torch.randn(3, 70, 5, 5, generator=torch.Generator().manual_seed(6))

    def grads(fn):
        x = inp.x.clone().requires_grad_()
        w = inp.wq.clone().requires_grad_()
        b = inp.bias.clone().requires_grad_()
        fn(x, w, b).backward(g)
        return x.grad, w.grad, b.grad

    got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
        x, w, inp.w_raw, b, stride, pad, "abs", 0.5, 32, 4, 0.25, in_bits=4,
        dac_bits=2, x_step=1.0 / 15))
    want = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bad,match", [
    (dict(sigma_mode=None, adc_bits=0), "neither"),
    (dict(differential=True), "differential"),
    (dict(in_bits=8, dac_bits=1), r"8 slices.*smallest dac_bits.*is 2"),
    (dict(in_bits=5, dac_bits=1), r"5 slices.*smallest dac_bits.*is 2"),
    (dict(in_bits=0), "in_bits"),
    (dict(in_bits=9, dac_bits=3), "in_bits"),
    (dict(in_bits=8, dac_bits=2, dtype=BF16), r"in_bits.*bfloat16"),
    (dict(dac_bits=-1), "dac_bits"),
    (dict(x_step=None), "x_step"),
    (dict(x_step=0.0), "x_step"),
    (dict(x_step=-0.5), "x_step"),
])
def test_argument_validation(bad, match):
    kw = dict(sigma_mode="abs", adc_bits=4, in_bits=4, dac_bits=2,
              x_step=0.25, differential=False, dtype=FP32)
    kw.update(bad)
    dtype = kw.pop("dtype")
    mode, bits = kw.pop("sigma_mode"), kw.pop("adc_bits")
    x, w = torch.rand(4, 96).to(dtype), torch.randn(8, 96).to(dtype)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_linear(x, w, w, None, mode, 0.5, 64, bits, 1.0, **kw)
    xc, wc = torch.rand(1, 4, 6, 6).to(dtype), torch.randn(8, 4, 3, 3).to(dtype)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_conv2d(xc, wc, wc, None, 1, 0, mode, 0.5, 64, bits, 1.0,
                              **kw)


def test_fp16_and_fp32_take_eight_bits_bf16_seven():
    for dtype, bits in ((FP16, 8), (FP32, 8), (BF16, 7)):
        x, w = torch.rand(4, 96).to(dtype), torch.randn(8, 96).to(dtype)
        out = ops.xbar_noisy_linear(x, w, w, None, None, 0.0, 64, 6, 1.0,
                                    in_bits=bits, dac_bits=2, x_step=1 / 255.)
        assert out.dtype == dtype and torch.isfinite(out.float()).all()


def test_dac_params_are_a_fill():
    p = ref_ops.xbar_dac_params(1.0 / 15.0, torch.device("cpu"))
    assert p.dtype == torch.float32 and p.shape == (2,)
    assert (float(p[0]), float(p[1])) == xso.dac_step(1.0 / 15.0)
    q = ref_ops.xbar_dac_params(torch.tensor([1.0 / 15.0]), torch.device("cpu"))
    assert torch.equal(p, q)


# ---------------------------------------------------------------------------
# flag and model
# ---------------------------------------------------------------------------


def _args(extra=()):
    argv = ['--n_train', '64', '--n_test', '32', '--batch_size', '8',
            '--nepochs', '1'] + list(extra)
    return broadcast_per_layer(build_noisynet_parser().parse_args(argv))


def test_flag_parses():
    assert _args().xbar_dac_bits == 0
    assert _args(['--xbar_dac_bits', '2']).xbar_dac_bits == 2


def test_quant_measure_records_its_range():
    from noisynet_amd.quant import QuantMeasure
    q = QuantMeasure(4, stochastic=0.0, max_value=5.0)
    assert q.last_range is None
    q(torch.rand(4, 8) * 5)
    assert q.last_range == (0.0, 5.0)


def test_model_serial_step_on_cpu(monkeypatch):
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
               '--xbar_dac_bits', '1', '--q_adc', '6', '--adc_max', '1'])
    seen = []
    real = ref_ops.xbar_vmm

    def spy(*args, **kw):
        seen.append((kw["in_bits"], kw["dac_bits"], float(kw["dac"][0])))
        return real(*args, **kw)

    monkeypatch.setattr(ref_ops, "xbar_vmm", spy)
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
    # every layer ran sliced, on the LSB of its own quantiser's range
    assert [s[:2] for s in seen] == [(4, 1)] * 4
    for k, s in enumerate(seen):
        lo, hi = getattr(m, 'quantize%d' % (k + 1)).last_range
        assert lo == 0.0 and hi > 0
        want = float(torch.tensor(max(hi / 15.0, 1e-6), dtype=torch.float32))
        assert s[2] == want, (k, s, want)


def test_serial_partials_are_smaller_than_unsliced_ones():
    outs = {}
    for D in (0, 1):
        a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
                   '--xbar_dac_bits', str(D)])
        torch.manual_seed(0)
        m = Net(a)
        m.train()
        torch.manual_seed(1)
        m(torch.rand(8, 3, 32, 32), 0, 0)
        outs[D] = m.partial_absmax[0][0]
    assert outs[1] < 0.5 * outs[0], outs


def test_dac_bits_zero_is_the_model_without_the_flag(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("bit-serial twin reached with --xbar_dac_bits 0")

    monkeypatch.setattr(ref_ops, "_xbar_vmm_serial", boom)
    outs = []
    for strip in (False, True):
        a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
                   '--q_adc', '6', '--adc_max', '3', '--xbar_dac_bits', '0'])
        if strip:   # an args object from before the flag existed
            delattr(a, 'xbar_dac_bits')
        torch.manual_seed(3)
        m = Net(a)
        m.train()
        torch.manual_seed(5)
        outs.append(m(torch.rand(8, 3, 32, 32), 0, 0))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("extra,match", [
    (['--xbar_dac_bits', '1', '--q_a', '4'], r"xbar_dac_bits needs --xbar_rows"),
    (['--xbar_rows', '64', '--xbar_dac_bits', '1', '--q_a', '4', '--xbar_diff',
      '--current', '1'], r"xbar_dac_bits.*xbar_diff"),
    (['--xbar_rows', '64', '--xbar_dac_bits', '1', '--current', '1'],
     r"q_a1 is 0"),
    (['--xbar_rows', '64', '--xbar_dac_bits', '1', '--q_a', '6',
      '--current', '1'], r"6 slices.*smallest --xbar_dac_bits.*is 2"),
    (['--xbar_rows', '64', '--xbar_dac_bits', '2', '--q_a', '8', '--bf16',
      '--current', '1'], r"q_a1 8 is too wide.*bf16"),
    (['--xbar_rows', '64', '--xbar_dac_bits', '-1', '--q_a', '4',
      '--current', '1'], r"xbar_dac_bits must be"),
])
def test_model_argument_validation(extra, match):
    with pytest.raises(ValueError, match=match):
        Net(_args(extra))


def test_model_refuses_a_layer_without_a_quantised_input():
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '64',
               '--xbar_dac_bits', '1'])
    a.q_a3 = 0
    with pytest.raises(ValueError, match=r"q_a3 is 0"):
        Net(a)


def test_model_refuses_a_range_that_does_not_start_at_zero():
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '64',
               '--xbar_dac_bits', '2'])
    m = Net(a)
    m.quantize2.min_value = -1.0
    m.quantize2.running_min.fill_(-1.0)
    m.quantize2.running_max.fill_(1.0)
    with pytest.raises(ValueError, match=r"quantize2.*range minimum"):
        m(torch.rand(2, 3, 32, 32), 0, 0)


def test_print_xbar_stats_names_the_slices(capsys):
    from noisynet_amd.drivers.cifar import print_xbar_stats
    a = _args(['--current', '1', '--q_a', '4', '--xbar_rows', '128',
               '--xbar_dac_bits', '1', '--q_adc', '6', '--adc_max', '1'])
    torch.manual_seed(0)
    m = Net(a)
    m(torch.rand(8, 3, 32, 32), 0, 0)
    print_xbar_stats(m, a)
    text = capsys.readouterr().out
    assert text.count("D=1 J=4") == 4 and "per slice" in text
