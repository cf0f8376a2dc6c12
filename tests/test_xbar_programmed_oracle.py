"""Programmed cells of the bit-sliced crossbars on the CPU: the reference twin
of the programming kernel and the ``cells=`` path of the pure-PyTorch op
against the fp64 oracle of xbar_programmed_oracle.py, the caps of the
configurations the GPU tests use, the flags, the model's programming schedule
and harness.test_cell_faults."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_cells_oracle as xco  # noqa: E402
import xbar_programmed_oracle as xpo  # noqa: E402
from noisynet_amd import harness, ops  # noqa: E402
from noisynet_amd.config import (broadcast_per_layer,  # noqa: E402
                                 build_noisynet_parser, xbar_cell_model)
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


# ---------------------------------------------------------------------------
# the test helper's Philox
# ---------------------------------------------------------------------------


def test_philox_known_answers():
    # Random123's known-answer vectors of philox4x32-10
    w = xpo.philox4x32(0, np.array([0], dtype=np.uint64))
    assert [int(v[0]) for v in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c,
                                      0x9b00dbd8]
    # counter (0xffffffff, 0xffffffff, 0, 0) is not a published vector; the
    # words must at least differ from the first and stay 32-bit
    w2 = xpo.philox4x32(0, np.array([2 ** 64 - 1], dtype=np.uint64))
    assert all(0 <= int(v[0]) < 2 ** 32 for v in w2)
    assert [int(v[0]) for v in w2] != [int(v[0]) for v in w]


# ---------------------------------------------------------------------------
# the reference twin of the programming kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xco.SHAPES))
def test_twin_ideal_chip_is_the_digits(shape, dtype):
    for B, E in ((4, 1), (4, 2), (6, 2), (7, 2), (4, 4)):
        inp = xco.general_inputs(shape, dtype, B)
        w = xco.general_w(B)
        G = ops.xbar_program_cells(inp.wq, B, E, w["w_step"], w["w_min"])
        assert G.dtype == dtype
        want = xpo.digits(inp.wq, w["w_step"], w["w_min"], B, E)
        assert G.shape == want.shape
        assert torch.equal(G.double(), want.double())


def test_twin_cell_statistics():
    wq = torch.full((256, 512), 5.0)              # every digit 1 (B 4, E 2)
    N = 2 * wq.numel()
    p_off, p_on = 0.05, 0.02
    G = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, 0.0, p_off, p_on, seed=3)
    assert set(G.unique().tolist()) == {0.0, 1.0, 3.0}
    for p, v in ((p_off, 0.0), (p_on, 3.0)):
        share = float((G == v).double().mean())
        assert abs(share - p) <= 5 * (p * (1 - p) / N) ** 0.5, (v, share)
    sigma = 0.1
    G = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, sigma, seed=3)
    r = G.double() - 1.0
    assert abs(float(r.mean())) <= 5 * sigma / N ** 0.5
    assert abs(float(r.std()) - sigma) <= 5 * sigma / (2 * N) ** 0.5
    again = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, sigma, seed=3)
    other = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, sigma, seed=4)
    assert torch.equal(G, again) and not torch.equal(G, other)
    # clamped at zero; a stuck-on cell varies like any other
    G = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, 0.5, seed=5)
    assert float(G.min()) == 0.0
    zeros = float((G == 0).double().mean())
    assert abs(zeros - 0.02275) <= 5 * (0.02275 * 0.97725 / N) ** 0.5
    G = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, sigma, 0.0, 1.0, seed=6)
    r = G.double() / 3.0 - 1.0
    assert abs(float(r.std()) - sigma) <= 5 * sigma / (2 * N) ** 0.5
    # one rounding: the bf16 chip is the fp32 chip rounded
    a = ops.xbar_program_cells(wq, 4, 2, 1.0, 0.0, sigma, 0.01, seed=7)
    b = ops.xbar_program_cells(wq.to(BF16), 4, 2, 1.0, 0.0, sigma, 0.01,
                               seed=7)
    assert torch.equal(a.to(BF16), b)


# ---------------------------------------------------------------------------
# the pure-PyTorch op on programmed cells against the oracle
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xpo.PROG_CFGS))
def test_cpu_op_on_cells_matches_oracle(shape, dtype):
    for cfg in xpo.PROG_CFGS[shape]:
        rows, bits, amax, B, E = cfg
        inp = xco.general_inputs(shape, dtype, B)
        w = xco.general_w(B)
        for bias in (True, False):
            r, G = xpo.twin_oracle(shape, dtype, cfg, xpo.GEN_SEEDS[0], bias)
            t = ops.XbarTelemetry()
            out = _call(shape, inp, None, 0.0, rows, bits, amax, bias=bias,
                        cell_bits=E, cells=G, want_telemetry=True,
                        telemetry_out=t, **w)
            assert out.dtype == dtype
            xco.assert_adc_close(out, r, rows, dtype, "cpu cells %s %s b%d"
                                 % (shape, cfg, bias))
            assert abs(float(t.partial_absmax) - r.absmax) <= 1e-5 * r.absmax
            assert abs(float(t.adc_clip_share) - xco.clip_share(r)) <= 0.01


def test_cpu_ideal_cells_are_the_digit_op():
    for shape in ("linear", "convA"):
        inp = xco.general_inputs(shape, FP32, 4)
        w = xco.general_w(4)
        G = ops.xbar_program_cells(inp.wq, 4, 2, w["w_step"], w["w_min"])
        for mode in ("abs", "abs2"):
            torch.manual_seed(8)
            a = _call(shape, inp, mode, 0.5, 64, 5, 2.0, cell_bits=2, **w)
            torch.manual_seed(8)
            b = _call(shape, inp, mode, 0.5, 64, 5, 2.0, cell_bits=2, cells=G,
                      **w)
            assert torch.equal(a, b), (shape, mode)


def test_cpu_noise_on_cells_does_not_fold_the_squares():
    # one-bit cells, abs2, sigma 0.3: s = sum x G^2 + sum x G, not 2 sum x G
    gen = torch.Generator().manual_seed(2)
    x = (torch.randint(0, 16, (1700, 96), generator=gen).float() / 15.0)
    wq = torch.randint(0, 16, (80, 96), generator=gen).float()
    inp = xpo.SimpleNamespace(x=x, wq=wq, bias=None)
    G = ops.xbar_program_cells(wq, 4, 1, 1.0, 0.0, 0.3, seed=1)
    r = xpo.blocked(x, G, None, "abs2", 32, 0, 0.0, 1.0, 0.0, 1)
    var = xco.noise_variance(r)
    folded = xpo.folded_variance("linear", inp, G, 32, 1.0, 0.0, 1)
    assert float((var / folded).mean()) > 1.03
    torch.manual_seed(4)
    out = ops.xbar_noisy_linear(x, wq, wq, None, "abs2", 0.5, 32, 0, 0.0,
                                w_bits=4, cell_bits=1, w_step=1.0, w_min=0.0,
                                cells=G)
    fo.check_noise_field(out, r.clean, var, 0.5,
                         stats=("mean", "std", "channel_std"),
                         what="cpu cells abs2 E=1")


def test_cpu_gradients_with_cells_are_those_of_the_plain_op():
    kind, xs, ws, stride, pad = xco.SHAPES["convA"]
    inp = xco.general_inputs("convA", FP32, 4)
    w = xco.general_w(4)
    G = ops.xbar_program_cells(inp.wq, 4, 2, w["w_step"], w["w_min"], 0.1,
                               0.02, 0.01, seed=1)
    g = torch.randn(3, 70, 5, 5, generator=torch.Generator().manual_seed(6))

    def grads(fn):
        x = inp.x.clone().requires_grad_()
        wt = inp.wq.clone().requires_grad_()
        b = inp.bias.clone().requires_grad_()
        fn(x, wt, b).backward(g)
        return x.grad, wt.grad, b.grad

    got = grads(lambda x, wt, b: ops.xbar_noisy_conv2d(
        x, wt, wt.detach(), b, stride, pad, "abs", 0.5, 32, 4, 2.0,
        cell_bits=2, cells=G, **w))
    want = grads(lambda x, wt, b: ops.conv2d(x, wt, b, stride, pad))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# the configurations of the GPU tests stay inside their caps (twin's G)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xpo.PROG_CFGS))
def test_programmed_cfgs_stay_inside_their_caps(shape, dtype):
    for cfg in xpo.PROG_CFGS[shape]:
        for gs in xpo.GEN_SEEDS:
            r, _ = xpo.twin_oracle(shape, dtype, cfg, gs)
            excluded, worst = xco.adc_report(r.out, r, cfg[0], dtype)
            clip = xco.clip_share(r)
            print("%s %s seed %d: excluded %.4f, clip share %.4f"
                  % (shape, cfg, gs, excluded, clip))
            assert worst == 0.0
            assert excluded <= 0.02 and 0.0 < clip < 0.5, (excluded, clip)


def test_the_cap_turns_a_candidate_down():
    shape, dtype, cfg = xpo.REJECTED_CFG
    r, _ = xpo.twin_oracle(shape, dtype, cfg, xpo.GEN_SEEDS[0])
    excluded, _ = xco.adc_report(r.out, r, cfg[0], dtype)
    print("rejected candidate: excluded %.4f, clip share %.4f"
          % (excluded, xco.clip_share(r)))
    assert excluded > 0.05 and not xco.clip_share(r) < 0.5
    with pytest.raises(AssertionError, match="rounding boundary"):
        xco.assert_adc_close(r.out, r, cfg[0], dtype, "rejected candidate")


# ---------------------------------------------------------------------------
# argument validation of the ops
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bad,match", [
    (dict(sigma=-0.1), "sigma"),
    (dict(p_stuck_off=-0.1), "p_stuck_off"),
    (dict(p_stuck_on=-0.1), "p_stuck_on"),
    (dict(p_stuck_off=0.6, p_stuck_on=0.5), r"p_stuck_off \+ p_stuck_on"),
    (dict(cell_bits=0), "cell_bits"),
    (dict(w_bits=9, cell_bits=3), "w_bits"),
    (dict(w_bits=7, cell_bits=1), "7 slices"),
])
def test_program_argument_validation(bad, match):
    kw = dict(w_bits=4, cell_bits=2, w_step=1.0 / 15, w_min=-0.5)
    kw.update(bad)
    with pytest.raises(ValueError, match=match):
        ops.xbar_program_cells(torch.randn(8, 96), **kw)


def test_cells_argument_validation():
    x, w = torch.rand(4, 96), torch.randn(8, 96)
    G = ops.xbar_program_cells(w, 4, 2, 1.0 / 15, -0.5, 0.1)
    kw = dict(w_bits=4, w_step=1.0 / 15, w_min=-0.5)
    with pytest.raises(ValueError, match=r"cells.*needs cell_bits"):
        ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0, cells=G)
    with pytest.raises(ValueError, match=r"cells.*shape"):
        ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0,
                              cell_bits=1, cells=G, **kw)
    with pytest.raises(ValueError, match=r"cells.*shape"):
        ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0,
                              cell_bits=2, cells=G[:, :, :64], **kw)


def test_defaults_never_reach_the_new_code(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("programmed-cell code reached with the flags "
                             "at their defaults")

    monkeypatch.setattr(ref_ops, "xbar_program_cells", boom)
    monkeypatch.setattr(ops.functional, "xbar_program_cells", boom)
    monkeypatch.setattr(ops, "xbar_program_cells", boom)
    outs = []
    for strip in (False, True):
        a = _args(['--current', '1', '--q_a', '4', '--q_w', '4',
                   '--xbar_rows', '128', '--q_adc', '6', '--adc_max', '3',
                   '--xbar_cell_bits', '2'])
        if strip:   # an args object from before the flags existed
            for f in ('xbar_cell_var', 'xbar_cell_stuck_off',
                      'xbar_cell_stuck_on', 'xbar_cell_seed'):
                delattr(a, f)
        torch.manual_seed(3)
        m = Net(a)
        m.train()
        torch.manual_seed(5)
        outs.append(m(torch.rand(8, 3, 32, 32), 0, 0))
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------
# flags, model, harness
# ---------------------------------------------------------------------------


def _args(extra=()):
    argv = ['--n_train', '64', '--n_test', '32', '--batch_size', '8',
            '--nepochs', '1'] + list(extra)
    return broadcast_per_layer(build_noisynet_parser().parse_args(argv))


BASE = ['--current', '1', '--q_a', '4', '--q_w', '4', '--xbar_rows', '128',
        '--xbar_cell_bits', '2', '--q_adc', '6', '--adc_max', '4']


def test_flag_defaults():
    a = _args()
    assert a.xbar_cell_var == 0.0 and a.xbar_cell_stuck_off == 0.0
    assert a.xbar_cell_stuck_on == 0.0 and a.xbar_cell_seed == -1
    assert xbar_cell_model(a) is None
    a = _args(BASE + ['--xbar_cell_var', '0.1', '--xbar_cell_stuck_off',
                      '0.02', '--xbar_cell_stuck_on', '0.01',
                      '--xbar_cell_seed', '7'])
    assert xbar_cell_model(a) == (0.1, 0.02, 0.01, 7)


@pytest.mark.parametrize("extra,match", [
    (['--xbar_cell_var', '0.1'], r"xbar_cell_var needs --xbar_cell_bits"),
    (['--xbar_cell_stuck_off', '0.1'],
     r"xbar_cell_stuck_off needs --xbar_cell_bits"),
    (['--xbar_cell_stuck_on', '0.1'],
     r"xbar_cell_stuck_on needs --xbar_cell_bits"),
    (['--xbar_rows', '64', '--current', '1', '--xbar_cell_var', '0.1'],
     r"xbar_cell_var needs --xbar_cell_bits"),
    (BASE + ['--xbar_cell_var', '-0.1'], r"xbar_cell_var must be >= 0"),
    (BASE + ['--xbar_cell_stuck_off', '-0.1'],
     r"xbar_cell_stuck_off must be >= 0"),
    (BASE + ['--xbar_cell_stuck_on', '-0.1'],
     r"xbar_cell_stuck_on must be >= 0"),
    (BASE + ['--xbar_cell_stuck_off', '0.6', '--xbar_cell_stuck_on', '0.5'],
     r"xbar_cell_stuck_off \+ --xbar_cell_stuck_on"),
    (BASE + ['--xbar_cell_var', '0.1', '--xbar_cell_seed', '-2'],
     r"xbar_cell_seed"),
])
def test_flag_validation(extra, match):
    with pytest.raises(ValueError, match=match):
        Net(_args(extra))


def test_model_programs_per_forward_in_training_and_once_in_eval(monkeypatch):
    calls = []
    real = ops.functional.xbar_program_cells

    def spy(wq, *a, **kw):
        calls.append(kw["seed"])
        return real(wq, *a, **kw)

    monkeypatch.setattr(ops, "xbar_program_cells", spy)
    a = _args(BASE + ['--xbar_cell_var', '0.1', '--xbar_cell_stuck_off',
                      '0.01'])
    torch.manual_seed(0)
    m = Net(a)
    x = torch.rand(8, 3, 32, 32)
    y = torch.randint(0, 10, (8,))
    m.train()
    loss = torch.nn.functional.cross_entropy(m(x, 0, 0), y)
    loss.backward()
    assert torch.isfinite(loss)
    for name in ('conv1', 'conv2', 'linear1', 'linear2'):
        g = getattr(m, name).weight.grad
        assert g is not None and torch.isfinite(g).all(), name
    m(x, 0, 0)
    assert calls == [None] * 8            # every layer, every forward, fresh
    # eval: one chip per evaluation, re-drawn by the next one
    del calls[:]
    m.eval()
    with torch.no_grad():
        e1 = m(x, 0, 30)
        e2 = m(x, 0, 30)
        assert len(calls) == 4
        m.eval()
        e3 = m(x, 0, 30)
        assert len(calls) == 8
        # a new weight version re-programs that layer alone
        m.conv2.weight.mul_(1.0)
        m(x, 0, 30)
        assert len(calls) == 9
    # a fixed chip: layer k of chip S uses seed 4 S + k
    del calls[:]
    a.xbar_cell_seed = 3
    m.eval()
    with torch.no_grad():
        m(x, 0, 30)
    assert calls == [12, 13, 14, 15]
    # with the noise on the outputs differ anyway; the chips must not
    assert e1.shape == e2.shape == e3.shape


def test_model_fixed_chip_is_reproducible_and_seeds_differ():
    # noise off (current 0), ADC on: the output is a function of the chip
    base = ['--q_a', '4', '--q_w', '4', '--xbar_rows', '128',
            '--xbar_cell_bits', '2', '--q_adc', '6', '--adc_max', '4',
            '--xbar_cell_var', '0.1']
    x = torch.rand(8, 3, 32, 32)
    outs = {}
    for seed in (3, 3, 4):
        a = _args(base + ['--xbar_cell_seed', str(seed)])
        torch.manual_seed(0)
        m = Net(a)
        m.eval()
        with torch.no_grad():
            m(x, 0, 30)
        # conv1's output: the logits of an untrained net are all zero
        outs.setdefault(seed, []).append(m.conv1_.clone())
    assert float(outs[3][0].abs().max()) > 0
    assert torch.equal(outs[3][0], outs[3][1])
    assert not torch.equal(outs[3][0], outs[4][0])


def test_print_xbar_stats_names_the_cell_model(capsys):
    from noisynet_amd.drivers.cifar import print_xbar_stats
    a = _args(BASE + ['--xbar_cell_var', '0.1', '--xbar_cell_stuck_off',
                      '0.02', '--xbar_cell_stuck_on', '0.01',
                      '--xbar_cell_seed', '5'])
    torch.manual_seed(0)
    m = Net(a)
    m(torch.rand(8, 3, 32, 32), 0, 0)
    print_xbar_stats(m, a)
    text = capsys.readouterr().out
    assert "σ_G 0.1" in text and "stuck off 0.02" in text
    assert "stuck on 0.01" in text and "chip seed 5" in text
    a.xbar_cell_seed = -1
    print_xbar_stats(m, a)
    assert "fresh per programming" in capsys.readouterr().out


def test_cell_faults_harness():
    a = _args(['--q_a', '4', '--q_w', '4', '--xbar_rows', '128',
               '--xbar_cell_bits', '2', '--q_adc', '6', '--adc_max', '4',
               '--xbar_cell_var', '0.05', '--xbar_cell_seed', '9'])
    torch.manual_seed(0)
    m = Net(a)
    m.train()
    gen = torch.Generator().manual_seed(1)
    val = (torch.rand(8, 3, 32, 32, generator=gen),
           torch.randint(0, 10, (8,), generator=gen))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    res = harness.test_cell_faults(m, a, val, [0.0, 0.2], [(0.05, 0.02)], 2)
    assert [(r["sigma"], r["p_stuck_off"], r["p_stuck_on"]) for r in res] \
        == [(0.0, 0.05, 0.02), (0.2, 0.05, 0.02)]
    for r in res:
        assert len(r["accs"]) == 2
        assert all(0.0 <= v <= 100.0 for v in r["accs"])
        assert r["min"] == min(r["accs"]) and r["max"] == max(r["accs"])
        assert abs(r["mean"] - sum(r["accs"]) / 2) <= 1e-9
        assert r["min"] <= r["mean"] <= r["max"]
    # the flags, the mode and the weights are as they were
    assert (a.xbar_cell_var, a.xbar_cell_stuck_off, a.xbar_cell_stuck_on,
            a.xbar_cell_seed) == (0.05, 0.0, 0.0, 9)
    assert m.training
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    # a single number is the stuck-off rate alone
    res = harness.test_cell_faults(m, a, val, [0.0], [0.1], 1)
    assert (res[0]["p_stuck_off"], res[0]["p_stuck_on"]) == (0.1, 0.0)
    a.xbar_cell_bits = 0
    a.xbar_cell_var = 0.0
    with pytest.raises(ValueError, match="xbar_cell_bits"):
        harness.test_cell_faults(m, a, val, [0.1], [0.0], 1)
