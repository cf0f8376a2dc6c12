"""The fused bit-serial tiled-crossbar kernel (per-slice noise + ADC,
xbar_serial_fwd_kernel) against the fp64 oracle of xbar_serial_oracle.py.

Shapes, inputs and configurations are those of xbar_serial_oracle (the shapes
of test_xbar_gpu.py, the smallest that cross every boundary of the 64x64x32
tile); test_xbar_serial_oracle.py asserts on the CPU that they exercise
clipping and ties and stay inside the boundary cap. Configurations read
(xbar_rows, adc_bits, adc_max, dac_bits); B = 4 throughout.
"""

import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_serial_oracle as xso  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
MODE_INT = {None: 0, "abs": 1, "abs2": 2}
FACTOR = 0.5
# relative error allowed on the float-atomic sum of sigma_abs: the bound of
# tests/test_fused_noise_gpu.py (TELE0_REL), whose reasoning applies unchanged
TELE0_REL = 2.8e-6
SHAPES = xso.SHAPES
NOISE_BATCH = {"linear": 1700, "convB": 200}      # >= 2^17 outputs each


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _dev(t):
    t = t.cuda()
    if t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


def _run(shape, inp, mode, rows, bits, amax, dac_bits, x_step, seed=1,
         telem=False, bias=True, factor=FACTOR, in_bits=4):
    """The C++ entry point itself (explicit seed). Returns (out, tele)."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    x, wq, wr = _dev(inp.x), _dev(inp.wq), _dev(inp.w_raw)
    b = inp.bias.cuda() if bias else torch.empty(0, device="cuda",
                                                 dtype=inp.x.dtype)
    f = torch.tensor([factor], device="cuda", dtype=torch.float32)
    adc = ops.reference.xbar_adc_params(bits, amax, x.device) \
        if 2 <= bits <= 16 else None
    if adc is None:
        adc = torch.empty(0, device="cuda", dtype=torch.float32)
    dac = ops.reference.xbar_dac_params(x_step, x.device)
    if kind == "conv":
        out, tele = ops.ext().xbar_serial_fwd_conv(
            x, wq, wr, b, stride, pad, MODE_INT[mode], f, rows, bits, adc,
            in_bits, dac_bits, dac, seed, telem)
    else:
        out, tele = ops.ext().xbar_serial_fwd_linear(
            x, wq, wr, b, MODE_INT[mode], f, rows, bits, adc, in_bits,
            dac_bits, dac, seed, telem)
    return out, tele.double().cpu()


# ---------------------------------------------------------------------------
# 1. exact: noise off, ADC on, x_step 1, power-of-two step
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_adc(shape, dtype):
    inp = xso.exact_inputs(shape, dtype)
    for rows, bits, amax, D in xso.EXACT_CFGS:
        ref = xso.oracle(shape, dtype, "exact", None, rows, bits, amax, D)
        out, _ = _run(shape, inp, None, rows, bits, amax, D, 1.0)
        assert out.dtype == dtype
        want = ref.out.to(dtype)          # fp32-exact, rounded once
        got = fo.to_mk(out).to(dtype)
        print("%s %s %s: clip share %.3f, tie share %.4f, mismatches %d"
              % (shape, _name(dtype), (rows, bits, amax, D),
                 xso.clip_share(ref), xso.tie_share(ref),
                 int((got != want).sum())))
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# 2. general inputs: noise off, ADC on
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xso.GENERAL_CFGS))
def test_general_adc(shape, dtype):
    inp = xso.general_inputs(shape, dtype)
    for rows, bits, amax, D in xso.GENERAL_CFGS[shape]:
        for bias in (True, False):
            ref = xso.oracle(shape, dtype, "general", None, rows, bits, amax,
                             D, bias)
            for telem in (False, True):
                out, _ = _run(shape, inp, None, rows, bits, amax, D,
                              1.0 / 15.0, telem=telem, bias=bias)
                xso.assert_adc_close(out, ref, rows, dtype, "%s %s %s b%d t%d"
                                     % (shape, _name(dtype),
                                        (rows, bits, amax, D), bias, telem))


# ---------------------------------------------------------------------------
# 3. ADC off, noise on: the shift-added noise field
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape,rows", [("linear", 64), ("convB", 32)])
def test_noise_field_sliced(shape, rows, mode, D):
    batch = NOISE_BATCH[shape]
    inp = xso.general_inputs(shape, BF16, batch=batch)
    ref = xso.oracle(shape, BF16, "general", mode, rows, 0, 0.0, D, True,
                     batch)
    assert ref.out.numel() >= 1 << 17 and ref.nblocks >= 3
    out, _ = _run(shape, inp, mode, rows, 0, 0.0, D, 1.0 / 15.0, seed=1234)
    fo.check_noise_field(out, ref.clean, xso.noise_variance(ref), FACTOR,
                         what="%s rows %d %s D=%d" % (shape, rows, mode, D))


# ---------------------------------------------------------------------------
# 4. slice draws are independent
# ---------------------------------------------------------------------------


def test_slice_draws_are_independent():
    # codes in {0, 15}, D = 1, one block: four equal slices. Independent
    # draws give variance (1 + 4 + 16 + 64) factor s_0 = 85 factor s_0, one
    # draw reused for every slice would give (1 + 2 + 4 + 8)^2 = 225
    gen = torch.Generator().manual_seed(9)
    M, K = 2000, 80
    x = torch.randint(0, 2, (M, 32), generator=gen).float()
    x[:, 0] = 1.0
    w = (torch.randn(K, 32, generator=gen) * 0.05).to(BF16)
    inp = SimpleNamespace(x=x.to(BF16), wq=w, w_raw=w, bias=None)
    xd, wd = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda")
    e = torch.empty(0, device="cuda")
    dac = ops.reference.xbar_dac_params(1.0 / 15.0, xd.device)
    out, _ = ops.ext().xbar_serial_fwd_linear(xd, wd, wd, e.to(BF16), 1, f,
                                              32, 0, e, 4, 1, dac, 77, False)
    ref = xso.linear_blocked(inp.x, inp.wq, inp.w_raw, None, "abs", 32, 0,
                             0.0, 1.0 / 15.0, 4, 1)
    assert ref.nblocks == 1 and ref.J == 4
    assert float((ref.s[0] - ref.s[3]).abs().max()) == 0.0
    var = xso.noise_variance(ref)
    assert float((var - 85.0 * ref.s[0]).abs().max()) <= 1e-9
    fo.check_noise_field(out, ref.clean, var, FACTOR,
                         stats=("mean", "std", "channel_std"),
                         what="four equal slices")


# ---------------------------------------------------------------------------
# 5. noise and ADC together
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_noise_goes_through_the_adc(shape, dtype, D):
    inp = xso.general_inputs(shape, dtype)
    rows, bits, amax = 64, 4, 1.75                # Qm 7 -> step 0.25
    ref = xso.oracle(shape, dtype, "general", "abs", rows, bits, amax, D,
                     False)
    assert ref.step == 0.25
    noisy, _ = _run(shape, inp, "abs", rows, bits, amax, D, 1.0 / 15.0,
                    seed=5, bias=False)
    clean, _ = _run(shape, inp, None, rows, bits, amax, D, 1.0 / 15.0,
                    seed=5, bias=False)
    o = fo.to_mk(noisy)
    k = o / ref.step
    # shift-adding multiples of a power-of-two step, rounded once to the
    # dtype, stays on the step's grid
    assert torch.equal(k, torch.round(k)), "output off the ADC grid"
    differ = float((o != fo.to_mk(clean)).double().mean())
    print("%s D=%d: %.3f of the outputs moved by the noise" % (shape, D,
                                                               differ))
    assert differ > 0.05


# ---------------------------------------------------------------------------
# 6. seeds
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_seeds(shape):
    inp = xso.general_inputs(shape, BF16)
    cfg = (64, 6, 0.5, 1, 1.0 / 15.0)
    a, _ = _run(shape, inp, "abs2", *cfg, seed=1001)
    b, _ = _run(shape, inp, "abs2", *cfg, seed=1001)
    c, _ = _run(shape, inp, "abs2", *cfg, seed=1002)
    assert torch.equal(a, b), "same seed, different output"
    assert float((a != c).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# 7. one slice is the unsliced kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_slice_is_the_unsliced_kernel(shape, dtype):
    # counter ((b*J + j)*M + m)*K + k with J = 1, x_step 1, on-grid codes
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = xso.exact_inputs(shape, dtype)
    rows, bits, amax = 64, 4, 56.0
    got, _ = _run(shape, inp, "abs", rows, bits, amax, 4, 1.0, seed=4242)
    x, wq, wr = _dev(inp.x), _dev(inp.wq), _dev(inp.w_raw)
    f = torch.tensor([FACTOR], device="cuda", dtype=torch.float32)
    adc = ops.reference.xbar_adc_params(bits, amax, x.device)
    if kind == "conv":
        want, _ = ops.ext().xbar_fwd_conv(x, wq, wr, inp.bias.cuda(), stride,
                                          pad, 1, f, rows, bits, adc, 4242,
                                          False)
    else:
        want, _ = ops.ext().xbar_fwd_linear(x, wq, wr, inp.bias.cuda(), 1, f,
                                            rows, bits, adc, 4242, False)
    assert torch.equal(got, want)
    # and the draw matters: another seed moves the output
    other, _ = _run(shape, inp, "abs", rows, bits, amax, 4, 1.0, seed=4243)
    assert float((other != want).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# 8. telemetry
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_adc_telemetry_exact(shape):
    inp = xso.exact_inputs(shape, BF16)
    for rows, bits, amax, D in xso.EXACT_CFGS:
        ref = xso.oracle(shape, BF16, "exact", None, rows, bits, amax, D)
        _, tele = _run(shape, inp, None, rows, bits, amax, D, 1.0, telem=True)
        assert tele.numel() == 5
        assert float(tele[0]) == 0.0 and float(tele[1]) == 0.0
        assert float(tele[2]) == float(ref.clean.max())
        assert float(tele[3]) == ref.clipped
        assert float(tele[4]) == ref.absmax
    # the public wrapper publishes the share over J * nblocks * M * K
    kind, xs, ws, stride, pad = SHAPES[shape]
    rows, bits, amax, D = xso.EXACT_CFGS[0]
    ref = xso.oracle(shape, BF16, "exact", None, rows, bits, amax, D)
    assert ref.n_partials == 4 * ref.nblocks * ref.out.numel()
    t = ops.XbarTelemetry()
    args = (_dev(inp.x), _dev(inp.wq), _dev(inp.w_raw), inp.bias.cuda())
    kw = dict(want_telemetry=True, telemetry_out=t, in_bits=4, dac_bits=D,
              x_step=1.0)
    if kind == "conv":
        ops.xbar_noisy_conv2d(*args, stride, pad, None, 0.0, rows, bits, amax,
                              **kw)
    else:
        ops.xbar_noisy_linear(*args, None, 0.0, rows, bits, amax, **kw)
    share = xso.clip_share(ref)
    assert abs(float(t.adc_clip_share) - share) <= 2.0 ** -22 * share
    assert float(t.partial_absmax) == ref.absmax
    assert t.power is None and t.nsr is None
    _, none = _run(shape, inp, None, rows, bits, amax, D, 1.0, telem=False)
    assert none.numel() == 0


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_noise_telemetry_slots(shape, mode, D):
    # ADC off, general inputs: sigma_abs is what the unsliced op reports
    inp = xso.general_inputs(shape, BF16)
    rows = 64
    ref = xso.oracle(shape, BF16, "general", mode, rows, 0, 0.0, D)
    out, tele = _run(shape, inp, mode, rows, 0, 0.0, D, 1.0 / 15.0, seed=31,
                     telem=True)
    o = fo.to_mk(out)
    s_abs = float(sum(sh * s for sh, s in zip(ref.shift, ref.s_abs)).sum())
    rel0 = abs(float(tele[0]) - s_abs) / s_abs
    A = sum(sh * a for sh, a in zip(ref.shift, ref.A)) + ref.bias_abs
    n = ref.n + ref.J * ref.nblocks + 2
    s1 = float((o - ref.clean).abs().sum())
    b1 = float((fo.U_OUT[BF16] * o.abs() + fo.gamma(n) * A).sum())
    bm = float(fo.det_bound(ref.clean, A, n, BF16).max())
    e1 = abs(float(tele[1]) - s1)
    e2 = abs(float(tele[2]) - float(ref.clean.max()))
    print("%s %s D=%d: tele0 rel %.3g, tele1 %.3g, tele2 %.3g of bound"
          % (shape, mode, D, rel0, e1 / b1, e2 / bm))
    assert rel0 <= TELE0_REL
    assert e1 <= b1 and e2 <= bm
    assert float(tele[3]) == 0.0
    # max |v_bj| includes the noise: within 6 sigma of the largest partial
    smax = float(max((FACTOR * s).sqrt().max() for s in ref.s))
    assert ref.absmax - 6 * smax <= float(tele[4]) <= ref.absmax + 6 * smax


# ---------------------------------------------------------------------------
# 9. backward and capture
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_is_the_plain_ops(shape):
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = xso.general_inputs(shape, BF16)

    def grads(fn):
        x = _dev(inp.x).requires_grad_()
        w = _dev(inp.wq).requires_grad_()
        b = inp.bias.cuda().requires_grad_()
        y = fn(x, w, b)
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(3))
        g = g.to(BF16).cuda()
        if g.dim() == 4:
            g = g.contiguous(memory_format=torch.channels_last)
        y.backward(g)
        return x.grad, w.grad, b.grad

    wr = _dev(inp.w_raw)
    kw = dict(in_bits=4, dac_bits=1, x_step=1.0 / 15.0)
    if kind == "conv":
        got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
            x, w, wr, b, stride, pad, "abs", FACTOR, 64, 4, 0.25, **kw))
        want = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    else:
        got = grads(lambda x, w, b: ops.xbar_noisy_linear(
            x, w, wr, b, "abs", FACTOR, 64, 4, 0.25, **kw))
        want = grads(lambda x, w, b: ops.linear(x, w, b))
    for name, a, b in zip(("gx", "gw", "gb"), got, want):
        assert torch.equal(a, b), name


def test_double_backward_runs():
    kind, xs, ws, stride, pad = SHAPES["convB"]
    inp = xso.general_inputs("convB", FP32)
    x = _dev(inp.x).requires_grad_()
    w = _dev(inp.wq).requires_grad_()
    y = ops.xbar_noisy_conv2d(x, w, _dev(inp.w_raw), None, stride, pad, "abs",
                              FACTOR, 64, 4, 0.25, in_bits=4, dac_bits=2,
                              x_step=1.0 / 15.0)
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    gx.square().sum().backward()
    assert w.grad is not None and torch.isfinite(w.grad).all()


def test_captured_call_draws_fresh_noise():
    from noisynet_amd.graphs import GraphedTrainStep
    inp = xso.general_inputs("linear", BF16)
    x, w, wr = _dev(inp.x), _dev(inp.wq), _dev(inp.w_raw)
    f = torch.tensor([FACTOR], device="cuda")
    torch.manual_seed(2)

    def body():
        return ops.xbar_noisy_linear(x, w, wr, None, "abs", f, 64, 6, 0.5,
                                     in_bits=4, dac_bits=1, x_step=1.0 / 15.0)

    gstep = GraphedTrainStep(body, warmup=1)
    first = gstep.replay().clone()
    second = gstep.replay().clone()
    gstep.close()
    torch.cuda.synchronize()
    assert torch.isfinite(first.float()).all()
    assert float((first != second).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# 10. argument validation in the C++ entry points
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_cpp_argument_validation(shape):
    inp = xso.general_inputs(shape, BF16)
    ok = (shape, inp, "abs", 64, 4, 1.0)
    with pytest.raises(RuntimeError, match="dac_bits"):
        _run(*ok, 0, 1.0 / 15.0)
    with pytest.raises(RuntimeError, match="dac_bits"):
        _run(*ok, -1, 1.0 / 15.0)
    with pytest.raises(RuntimeError, match="in_bits"):
        _run(*ok, 1, 1.0 / 15.0, in_bits=0)
    with pytest.raises(RuntimeError, match="in_bits"):
        _run(*ok, 3, 1.0 / 15.0, in_bits=9)
    with pytest.raises(RuntimeError, match="in_bits"):       # bf16: <= 7
        _run(*ok, 2, 1.0 / 15.0, in_bits=8)
    with pytest.raises(RuntimeError, match=r"7 slices.*smallest.*is 2"):
        _run(*ok, 1, 1.0 / 15.0, in_bits=7)
    with pytest.raises(RuntimeError, match="xbar_rows"):
        _run(shape, inp, "abs", 48, 4, 1.0, 1, 1.0 / 15.0)
    with pytest.raises(RuntimeError, match="both off"):
        _run(shape, inp, None, 64, 0, 0.0, 1, 1.0 / 15.0)
    inp32 = xso.general_inputs(shape, FP32)
    out, _ = _run(shape, inp32, "abs", 64, 4, 1.0, 2, 1.0 / 255.0, in_bits=8)
    assert torch.isfinite(out).all()
    x, w = _dev(inp.x), _dev(inp.wq)
    with pytest.raises(ValueError, match="differential"):
        if x.dim() == 4:
            ops.xbar_noisy_conv2d(x, w, w, None, 2, 2, "abs", 0.5, 64, 4, 1.0,
                                  differential=True, in_bits=4, dac_bits=1,
                                  x_step=1.0 / 15.0)
        else:
            ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0,
                                  differential=True, in_bits=4, dac_bits=1,
                                  x_step=1.0 / 15.0)


# ---------------------------------------------------------------------------
# 11. model
# ---------------------------------------------------------------------------


def _model(extra, seed=0):
    from noisynet_amd import utils
    from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser
    from noisynet_amd.models.noisynet import Net
    args = build_noisynet_parser().parse_args(
        ['--current', '1', '--q_a', '4', '--bf16', '--batch_size', '8']
        + extra)
    broadcast_per_layer(args)
    torch.manual_seed(seed)
    model = Net(args)
    utils.init_model(model, args)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.float()
    return model.to(memory_format=torch.channels_last)


def _batch():
    gen = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 16, (8, 3, 32, 32), generator=gen).float() / 15)
    x = x.cuda().bfloat16().contiguous(memory_format=torch.channels_last)
    return x, torch.randint(0, 10, (8,), generator=gen).cuda()


def test_model_trains_a_step_on_bit_serial_crossbars():
    model = _model(['--xbar_rows', '128', '--xbar_dac_bits', '1', '--q_adc',
                    '6', '--adc_max', '1'])
    model.train()
    x, y = _batch()
    loss = ops.cross_entropy(model(x, 0, 0), y)
    loss.backward()
    assert torch.isfinite(loss)
    for name in ('conv1', 'conv2', 'linear1', 'linear2'):
        g = getattr(model, name).weight.grad
        assert g is not None and torch.isfinite(g.float()).all(), name
    for k in range(4):
        assert len(model.adc_clip[k]) == 1
        assert 0.0 <= model.adc_clip[k][0] <= 1.0
        assert model.partial_absmax[k][0] > 0
        assert len(model.power[k]) == 1
