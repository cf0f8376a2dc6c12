"""Bit-sliced crossbar weights on the CPU: the pure-PyTorch op against the
fp64 oracle of xbar_cells_oracle.py, the digit decomposition the mode rests
on, the argument rules, the flag and the model wiring."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_cells_oracle as xco  # noqa: E402
from noisynet_amd import ops  # noqa: E402
from noisynet_amd.config import (broadcast_per_layer,  # noqa: E402
                                 build_noisynet_parser)
from noisynet_amd.models.noisynet import Net  # noqa: E402
from noisynet_amd.ops import reference as ref_ops  # noqa: E402

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _call(shape, inp, mode, factor, rows, bits, amax, bias=True, **kw):
    kind, xs, ws, stride, pad = xco.SHAPES[shape]
    b = inp.bias if bias else None
    if kind == "conv":
        return ops.xbar_noisy_conv2d(inp.x, inp.wq, inp.wq, b, stride, pad,
                                     mode, factor, rows, bits, amax, **kw)
    return ops.xbar_noisy_linear(inp.x, inp.wq, inp.wq, b, mode, factor, rows,
                                 bits, amax, **kw)


def _rows(shape, inp):
    kind, xs, ws, stride, pad = xco.SHAPES[shape]
    if kind == "conv":
        return xco.xo.conv_rows(inp.x, ws[2], ws[3], stride, pad)
    return inp.x.double()


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=_name)
@pytest.mark.parametrize("B,E", [(4, 1), (4, 2), (4, 4), (6, 2), (7, 2),
                                 (5, 3), (3, 1)])
def test_digits_reconstruct_the_grid_weight(B, E, dtype):
    inp = xco.general_inputs("linear", dtype, B)
    w = xco.general_w(B)
    r = xco.oracle("linear", dtype, "general", None, 64, 0, 0.0, B, E)
    T = -(-B // E)
    assert r.T == T
    digits = [(r.code >> (t * E)) & (2 ** E - 1) for t in range(T)]
    assert all(int(d.min()) >= 0 and int(d.max()) <= 2 ** E - 1
               for d in digits)
    code = sum(d << (t * E) for t, d in enumerate(digits))
    assert torch.equal(code, r.code)
    assert int(r.code.min()) == 0 and int(r.code.max()) == 2 ** B - 1
    # the grid weight is the quantiser's output before the dtype rounding:
    # within one rounding of the stored weight, and half a step apart at most
    ws, _, wm = xco.cell_params(w["w_step"], w["w_min"])
    grid = wm + code.double() * ws
    stored = inp.wq.double()
    assert float((grid - stored).abs().max()) \
        <= 0.5 * fo.U_OUT[dtype] + 2.0 ** -24
    fq = ref_ops.fake_quant_forward(fo.make_inputs(
        *xco.SHAPES["linear"][1:3], dtype, 1).wq.float(), B, -0.5, 0.5, 0)
    assert float((grid - fq.double()).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("shape", list(xco.SHAPES))
@pytest.mark.parametrize("B,E", [(4, 1), (4, 2), (6, 2), (4, 4)])
def test_oracle_without_noise_and_adc_is_the_grid_matmul(shape, B, E):
    for dtype in (BF16, FP32):
        inp = xco.general_inputs(shape, dtype, B)
        r = xco.oracle(shape, dtype, "general", None, 64, 0, 0.0, B, E)
        kind, xs, ws, stride, pad = xco.SHAPES[shape]
        want = _rows(shape, inp) @ r.w_grid.t() + inp.bias.double()
        assert float((r.out - want).abs().max()) <= 1e-11
        assert float((r.out - r.clean).abs().max()) == 0.0


def test_oracle_noise_variance_is_shift_weighted():
    r1 = xco.oracle("linear", FP32, "general", "abs", 64, 0, 0.0, 4, 4)
    for E in (1, 2):
        r = xco.oracle("linear", FP32, "general", "abs", 64, 0, 0.0, 4, E)
        # abs: s_bt = p_bt, so sum 2^(tE) s_bt is the one-slice current and
        # the variance sum 4^(tE) s_bt stays below it times 2^((T-1)E)
        lin = sum(sh * s for sh, s in zip(r.shift, r.s))
        assert float((lin - sum(r1.s)).abs().max()) <= 1e-9
        var = xco.noise_variance(r)
        assert float((var - lin).min()) >= -1e-12
        assert float((var - r.shift[-1] * lin).max()) <= 1e-9


# ---------------------------------------------------------------------------
# the pure-PyTorch op against the oracle, noise off
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xco.GENERAL_CFGS))
def test_cpu_op_matches_oracle(shape, dtype):
    for rows, bits, amax, B, E in xco.GENERAL_CFGS[shape]:
        inp = xco.general_inputs(shape, dtype, B)
        w = xco.general_w(B)
        for bias in (True, False):
            r = xco.oracle(shape, dtype, "general", None, rows, bits, amax, B,
                           E, bias)
            t = ops.XbarTelemetry()
            out = _call(shape, inp, None, 0.0, rows, bits, amax, bias=bias,
                        cell_bits=E, want_telemetry=True, telemetry_out=t,
                        **w)
            assert out.dtype == dtype
            xco.assert_adc_close(out, r, rows, dtype, "cpu %s %s b%d" % (
                shape, (rows, bits, amax, B, E), bias))
            assert abs(float(t.partial_absmax) - r.absmax) <= 1e-5 * r.absmax
            assert abs(float(t.adc_clip_share) - xco.clip_share(r)) <= 0.01
            assert t.power is None and t.nsr is None


def test_cpu_exact_case_is_bit_equal():
    for shape in xco.SHAPES:
        inp = xco.exact_inputs(shape, FP32)
        for rows, bits, amax, E in xco.EXACT_CFGS:
            r = xco.oracle(shape, FP32, "exact", None, rows, bits, amax, 4, E)
            t = ops.XbarTelemetry()
            out = _call(shape, inp, None, 0.0, rows, bits, amax, cell_bits=E,
                        want_telemetry=True, telemetry_out=t, **xco.EXACT_W)
            assert torch.equal(fo.to_mk(out), r.out)
            assert float(t.partial_absmax) == r.absmax
            share = xco.clip_share(r)
            assert abs(float(t.adc_clip_share) - share) <= 2.0 ** -22 * share


def test_cpu_op_without_noise_and_adc_is_the_grid_matmul():
    # factor 0 switches the noise off without tripping the "both off" rule
    for shape in ("linear", "convA"):
        inp = xco.general_inputs(shape, BF16, 6)
        r = xco.oracle(shape, BF16, "general", None, 64, 0, 0.0, 6, 2)
        out = _call(shape, inp, "abs2", 0.0, 64, 0, 0.0, cell_bits=2,
                    **xco.general_w(6))
        A = sum(sh * a for sh, a in zip(r.shift, r.A)) \
            + abs(r.w_min) * r.xabs + r.bias_abs
        fo.assert_within(out, r.out, fo.det_bound(
            r.out, A, r.n + (r.T + 1) * r.nblocks + 2, BF16),
            "%s grid matmul" % shape)
        # and it is NOT the matmul with the dtype-rounded weights
        kind, xs, ws, stride, pad = xco.SHAPES[shape]
        stored = _rows(shape, inp) @ xco.xo.weight_rows(inp.wq).t() \
            + inp.bias.double()
        assert float((stored - r.out).abs().max()) > 1e-4


# ---------------------------------------------------------------------------
# the inputs chosen for the GPU tests stay inside their caps (oracle alone)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cfg", xco.EXACT_CFGS)
def test_exact_inputs_exercise_clipping_and_ties(cfg):
    rows, bits, amax, E = cfg
    r = xco.oracle("linear", FP32, "exact", None, rows, bits, amax, 4, E)
    clip, ties = xco.clip_share(r), xco.tie_share(r)
    print("%s: clip share %.3f, tie share %.4f" % (cfg, clip, ties))
    assert clip > 0.01 and ties > 0.002, (clip, ties)
    assert r.step == 2.0 ** round(torch.log2(torch.tensor(r.step)).item())


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xco.GENERAL_CFGS))
def test_general_inputs_stay_inside_their_caps(shape, dtype):
    for cfg in xco.GENERAL_CFGS[shape]:
        rows, bits, amax, B, E = cfg
        for bias in (True, False):
            r = xco.oracle(shape, dtype, "general", None, rows, bits, amax, B,
                           E, bias)
            excluded, worst = xco.adc_report(r.out, r, rows, dtype)
            clip = xco.clip_share(r)
            print("%s %s: excluded %.4f, clip share %.4f" % (shape, cfg,
                                                            excluded, clip))
            assert worst == 0.0
            assert excluded <= 0.05 and clip > 0.005, (excluded, clip)


def test_the_cap_turns_a_tie_heavy_config_down():
    shape, dtype, (rows, bits, amax, B, E) = xco.REJECTED_CFG
    r = xco.oracle(shape, dtype, "general", None, rows, bits, amax, B, E)
    excluded, _ = xco.adc_report(r.out, r, rows, dtype)
    print("rejected candidate: excluded %.4f" % excluded)
    assert excluded > 0.05
    with pytest.raises(AssertionError, match="rounding boundary"):
        xco.assert_adc_close(r.out, r, rows, dtype, "rejected candidate")


# ---------------------------------------------------------------------------
# noise on the CPU path
# ---------------------------------------------------------------------------


def test_cpu_slice_noise_variance():
    # every code 0b0101, E = 2, one block: two equal slices, independent
    # draws shift-added give variance (1 + 16) * factor * s_0 (25x if one draw
    # served both slices)
    gen = torch.Generator().manual_seed(9)
    M, K = 2000, 80
    x = torch.randint(0, 16, (M, 32), generator=gen).float() / 15.0
    x[:, 0] = 1.0
    w = torch.full((K, 32), 5.0)
    r = xco.linear_blocked(x, w, None, "abs", 32, 0, 0.0, 1.0, 0.0, 4, 2)
    assert r.nblocks == 1 and r.T == 2
    assert float((r.s[0] - r.s[1]).abs().max()) == 0.0
    var = xco.noise_variance(r)
    assert float((var - 17.0 * r.s[0]).abs().max()) <= 1e-9
    torch.manual_seed(11)
    out = ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 32, 0, 0.0,
                                w_bits=4, cell_bits=2, w_step=1.0, w_min=0.0)
    fo.check_noise_field(out, r.clean, var, 0.5,
                         stats=("mean", "std", "channel_std"),
                         what="cpu two equal slices")


def test_cpu_gradients_are_those_of_the_plain_op():
    kind, xs, ws, stride, pad = xco.SHAPES["convA"]
    inp = xco.general_inputs("convA", FP32, 4)
    g = torch.randn(3, 70, 5, 5, generator=torch.Generator().manual_seed(6))

    def grads(fn):
        x = inp.x.clone().requires_grad_()
        w = inp.wq.clone().requires_grad_()
        b = inp.bias.clone().requires_grad_()
        fn(x, w, b).backward(g)
        return x.grad, w.grad, b.grad

    got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
        x, w, w.detach(), b, stride, pad, "abs", 0.5, 32, 4, 2.0, cell_bits=2,
        **xco.general_w(4)))
    want = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bad,match", [
    (dict(sigma_mode=None, adc_bits=0), "neither"),
    (dict(differential=True), r"differential.*accumulator sets.*follow-up"),
    (dict(in_bits=4, dac_bits=1, x_step=0.1),
     r"dac_bits.*accumulator sets.*follow-up"),
    (dict(w_bits=8, cell_bits=1), r"8 slices.*smallest cell_bits.*is 2"),
    (dict(w_bits=5, cell_bits=1), r"5 slices.*smallest cell_bits.*is 2"),
    (dict(w_bits=0), "w_bits"),
    (dict(w_bits=9, cell_bits=3), "w_bits"),
    (dict(cell_bits=5), "cell_bits"),
    (dict(cell_bits=-1), "cell_bits"),
    (dict(w_step=None), "w_step"),
    (dict(w_min=None), "w_min"),
    (dict(w_step=0.0), "w_step"),
    (dict(w_step=-0.5), "w_step"),
])
def test_argument_validation(bad, match):
    kw = dict(sigma_mode="abs", adc_bits=4, w_bits=4, cell_bits=2,
              w_step=1.0 / 15, w_min=-0.5, differential=False)
    kw.update(bad)
    mode, bits = kw.pop("sigma_mode"), kw.pop("adc_bits")
    x, w = torch.rand(4, 96), torch.randn(8, 96)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_linear(x, w, w, None, mode, 0.5, 64, bits, 1.0, **kw)
    xc, wc = torch.rand(1, 4, 6, 6), torch.randn(8, 4, 3, 3)
    with pytest.raises(ValueError, match=match):
        ops.xbar_noisy_conv2d(xc, wc, wc, None, 1, 0, mode, 0.5, 64, bits, 1.0,
                              **kw)


def test_cell_bits_zero_never_reaches_the_new_code(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("cell-sliced code reached with cell_bits 0")

    monkeypatch.setattr(ref_ops, "_xbar_vmm_cells", boom)
    monkeypatch.setattr(ref_ops, "xbar_check_cell_args", boom)
    monkeypatch.setattr(ref_ops, "xbar_cell_params", boom)
    x, w = torch.rand(4, 96), torch.randn(8, 96)
    torch.manual_seed(4)
    a = ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0)
    torch.manual_seed(4)
    b = ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0,
                              w_bits=4, cell_bits=0, w_step=0.1, w_min=-0.5)
    assert torch.equal(a, b)


def test_cell_params_are_a_fill():
    p = ref_ops.xbar_cell_params(1.0 / 15.0, -0.5, torch.device("cpu"))
    assert p.dtype == torch.float32 and p.shape == (3,)
    assert tuple(float(v) for v in p) == xco.cell_params(1.0 / 15.0, -0.5)
    q = ref_ops.xbar_cell_params(torch.tensor([1.0 / 15.0]),
                                 torch.tensor(-0.5), torch.device("cpu"))
    assert torch.equal(p, q)


# ---------------------------------------------------------------------------
# flag and model
# ---------------------------------------------------------------------------


def _args(extra=()):
    argv = ['--n_train', '64', '--n_test', '32', '--batch_size', '8',
            '--nepochs', '1'] + list(extra)
    return broadcast_per_layer(build_noisynet_parser().parse_args(argv))


def test_flag_parses():
    assert _args().xbar_cell_bits == 0
    assert _args(['--xbar_cell_bits', '2']).xbar_cell_bits == 2


def test_model_cells_step_on_cpu(monkeypatch):
    a = _args(['--current', '1', '--q_a', '4', '--q_w', '4', '--xbar_rows',
               '128', '--xbar_cell_bits', '2', '--q_adc', '6', '--adc_max',
               '4'])
    seen = []
    real = ref_ops.xbar_vmm

    def spy(*args, **kw):
        seen.append((kw["w_bits"], kw["cell_bits"],
                     tuple(float(v) for v in kw["cell"])))
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
    # every layer ran sliced, on the grid of its own weight quantiser
    assert [s[:2] for s in seen] == [(4, 2)] * 4
    for k, name in enumerate(('conv1', 'conv2', 'linear1', 'linear2')):
        lo, hi = getattr(m, name).quantize_weights.last_range
        assert seen[k][2] == xco.cell_params(xco.grid_step(4, lo, hi), lo)


def test_offset_binary_cells_draw_more_current_than_signed_ones():
    power = {}
    for E in (0, 2):
        a = _args(['--current', '1', '--q_a', '4', '--q_w', '4',
                   '--xbar_rows', '128', '--xbar_cell_bits', str(E)])
        torch.manual_seed(0)
        m = Net(a)
        m.train()
        torch.manual_seed(1)
        m(torch.rand(8, 3, 32, 32), 0, 0)
        power[E] = m.power[1][0]
    assert power[2] > power[0], power


def test_cell_bits_zero_is_the_model_without_the_flag(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("cell-sliced twin reached with --xbar_cell_bits 0")

    monkeypatch.setattr(ref_ops, "_xbar_vmm_cells", boom)
    outs = []
    for strip in (False, True):
        a = _args(['--current', '1', '--q_a', '4', '--q_w', '4',
                   '--xbar_rows', '128', '--q_adc', '6', '--adc_max', '3',
                   '--xbar_cell_bits', '0'])
        if strip:   # an args object from before the flag existed
            delattr(a, 'xbar_cell_bits')
        torch.manual_seed(3)
        m = Net(a)
        m.train()
        torch.manual_seed(5)
        outs.append(m(torch.rand(8, 3, 32, 32), 0, 0))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("extra,match", [
    (['--xbar_cell_bits', '2', '--q_w', '4'],
     r"xbar_cell_bits needs --xbar_rows"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '2', '--q_w', '4',
      '--xbar_diff', '--current', '1'], r"xbar_cell_bits.*xbar_diff"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '2', '--q_w', '4', '--q_a',
      '4', '--xbar_dac_bits', '1', '--current', '1'],
     r"xbar_cell_bits.*xbar_dac_bits"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '2', '--q_w', '4',
      '--current', '1', '--print_stats'], r"print_stats"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '2', '--current', '1'],
     r"q_w1 is 0"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '2', '--q_w', '8',
      '--current', '1'], r"q_w1 is 8"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '1', '--q_w', '6',
      '--current', '1'], r"6 slices.*smallest --xbar_cell_bits.*is 2"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '5', '--q_w', '4',
      '--current', '1'], r"xbar_cell_bits must be"),
    (['--xbar_rows', '64', '--xbar_cell_bits', '-1', '--q_w', '4',
      '--current', '1'], r"xbar_cell_bits must be"),
])
def test_model_argument_validation(extra, match):
    with pytest.raises(ValueError, match=match):
        Net(_args(extra))


def test_model_refuses_a_layer_without_quantised_weights():
    a = _args(['--current', '1', '--q_w', '4', '--xbar_rows', '64',
               '--xbar_cell_bits', '2'])
    a.q_w3 = 0
    with pytest.raises(ValueError, match=r"q_w3 is 0"):
        Net(a)


def test_model_refuses_a_range_the_dtype_cannot_carry():
    # 7-bit codes over [-100, -50]: step 0.394, but bf16 moves a weight near
    # -100 by up to 100 * 2^-8 = 0.39 >= step / 2
    a = _args(['--current', '1', '--q_w', '7', '--xbar_rows', '64',
               '--xbar_cell_bits', '2'])
    m = Net(a)
    m.conv2.quantize_weights._range_cache = (-100.0, -50.0)
    x = torch.rand(2, 3, 32, 32)
    m(x, 0, 0)                                      # fp32 carries the codes
    m = m.bfloat16()
    with pytest.raises(ValueError, match=r"layer 2.*cannot be recovered"):
        m(x.bfloat16(), 0, 0)


def test_print_xbar_stats_names_the_cell_slices(capsys):
    from noisynet_amd.drivers.cifar import print_xbar_stats
    a = _args(['--current', '1', '--q_a', '4', '--q_w', '4', '--xbar_rows',
               '128', '--xbar_cell_bits', '2', '--q_adc', '6', '--adc_max',
               '4'])
    torch.manual_seed(0)
    m = Net(a)
    m(torch.rand(8, 3, 32, 32), 0, 0)
    print_xbar_stats(m, a)
    text = capsys.readouterr().out
    assert text.count("E=2 T=2") == 4 and "per cell slice" in text
