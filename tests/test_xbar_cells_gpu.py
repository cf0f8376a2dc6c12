"""The fused bit-sliced-weight tiled-crossbar kernel (per-slice noise +
unipolar ADC, xbar_cells_fwd_kernel) against the fp64 oracle of
xbar_cells_oracle.py.

Shapes, inputs and configurations are those of xbar_cells_oracle (the shapes
of test_xbar_gpu.py, the smallest that cross every boundary of the 64x64x32
tile); test_xbar_cells_oracle.py asserts on the CPU that they exercise
clipping and ties and stay inside the boundary cap. Exact configurations read
(xbar_rows, adc_bits, adc_max, cell_bits) with B = 4, general ones
(xbar_rows, adc_bits, adc_max, w_bits, cell_bits).
"""

import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_cells_oracle as xco  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
MODE_INT = {None: 0, "abs": 1, "abs2": 2}
FACTOR = 0.5
# relative error allowed on the float-atomic sum of the cell current: the
# bound of tests/test_fused_noise_gpu.py (TELE0_REL), whose reasoning applies
# unchanged
TELE0_REL = 2.8e-6
SHAPES = xco.SHAPES
NOISE_BATCH = {"linear": 1700, "convB": 200}      # >= 2^17 outputs each


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _dev(t):
    t = t.cuda()
    if t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


def _run(shape, inp, mode, rows, bits, amax, w_bits, cell_bits, w_step, w_min,
         seed=1, telem=False, bias=True, factor=FACTOR):
    """The C++ entry point itself (explicit seed). Returns (out, tele)."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    x, wq = _dev(inp.x), _dev(inp.wq)
    b = inp.bias.cuda() if bias else torch.empty(0, device="cuda",
                                                 dtype=inp.x.dtype)
    f = torch.tensor([factor], device="cuda", dtype=torch.float32)
    adc = ops.reference.xbar_adc_params(bits, amax, x.device, unipolar=True) \
        if 2 <= bits <= 16 else None
    if adc is None:
        adc = torch.empty(0, device="cuda", dtype=torch.float32)
    cell = ops.reference.xbar_cell_params(w_step, w_min, x.device)
    if kind == "conv":
        out, tele = ops.ext().xbar_cells_fwd_conv(
            x, wq, b, stride, pad, MODE_INT[mode], f, rows, bits, adc, w_bits,
            cell_bits, cell, seed, telem)
    else:
        out, tele = ops.ext().xbar_cells_fwd_linear(
            x, wq, b, MODE_INT[mode], f, rows, bits, adc, w_bits, cell_bits,
            cell, seed, telem)
    return out, tele.double().cpu()


def _exact(shape, inp, mode, rows, bits, amax, E, **kw):
    return _run(shape, inp, mode, rows, bits, amax, 4, E, 1.0, -8.0, **kw)


def _general(shape, inp, mode, rows, bits, amax, B, E, **kw):
    w = xco.general_w(B)
    return _run(shape, inp, mode, rows, bits, amax, B, E, w["w_step"],
                w["w_min"], **kw)


# ---------------------------------------------------------------------------
# 1. exact: noise off, ADC on, w_step 1, power-of-two step
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_adc(shape, dtype):
    inp = xco.exact_inputs(shape, dtype)
    for rows, bits, amax, E in xco.EXACT_CFGS:
        ref = xco.oracle(shape, dtype, "exact", None, rows, bits, amax, 4, E)
        out, _ = _exact(shape, inp, None, rows, bits, amax, E)
        assert out.dtype == dtype
        want = ref.out.to(dtype)          # fp32-exact, rounded once
        got = fo.to_mk(out).to(dtype)
        print("%s %s %s: clip share %.3f, tie share %.4f, mismatches %d"
              % (shape, _name(dtype), (rows, bits, amax, E),
                 xco.clip_share(ref), xco.tie_share(ref),
                 int((got != want).sum())))
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------
# 2. general inputs: noise off, ADC on
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(xco.GENERAL_CFGS))
def test_general_adc(shape, dtype):
    for rows, bits, amax, B, E in xco.GENERAL_CFGS[shape]:
        inp = xco.general_inputs(shape, dtype, B)
        for bias in (True, False):
            ref = xco.oracle(shape, dtype, "general", None, rows, bits, amax,
                             B, E, bias)
            for telem in (False, True):
                out, _ = _general(shape, inp, None, rows, bits, amax, B, E,
                                  telem=telem, bias=bias)
                xco.assert_adc_close(out, ref, rows, dtype, "%s %s %s b%d t%d"
                                     % (shape, _name(dtype),
                                        (rows, bits, amax, B, E), bias, telem))


# ---------------------------------------------------------------------------
# 3. ADC off, noise on: the shift-added noise field
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape,rows", [("linear", 64), ("convB", 32)])
def test_noise_field_sliced(shape, rows, mode, E):
    batch = NOISE_BATCH[shape]
    inp = xco.general_inputs(shape, BF16, 4, batch=batch)
    ref = xco.oracle(shape, BF16, "general", mode, rows, 0, 0.0, 4, E, True,
                     batch)
    assert ref.out.numel() >= 1 << 17 and ref.nblocks >= 3
    out, _ = _general(shape, inp, mode, rows, 0, 0.0, 4, E, seed=1234)
    fo.check_noise_field(out, ref.clean, xco.noise_variance(ref), FACTOR,
                         what="%s rows %d %s E=%d" % (shape, rows, mode, E))


def test_fp32_abs2_four_slices_uses_the_large_lds():
    # the one case whose tiles pass 64 KB (82944 bytes): fp32, four slices of
    # multi-bit cells (one-bit cells need no squares tiles), abs2
    inp = xco.general_inputs("convA", FP32, 7)
    ref = xco.oracle("convA", FP32, "general", "abs2", 64, 0, 0.0, 7, 2)
    assert ref.T == 4
    out, _ = _general("convA", inp, "abs2", 64, 0, 0.0, 7, 2, factor=0.0)
    A = sum(sh * a for sh, a in zip(ref.shift, ref.A)) \
        + abs(ref.w_min) * ref.xabs + ref.bias_abs
    fo.assert_within(out, ref.clean, fo.det_bound(
        ref.clean, A, ref.n + (ref.T + 1) * ref.nblocks + 2, FP32),
        "fp32 abs2 four slices, factor 0")


# ---------------------------------------------------------------------------
# 4. slice draws are independent
# ---------------------------------------------------------------------------


def test_slice_draws_are_independent():
    # every code 0b0101, E = 2, one block: two equal slices. Independent
    # draws give variance (1 + 16) factor s_0 = 17 factor s_0, one draw
    # reused for both slices would give (1 + 4)^2 = 25
    gen = torch.Generator().manual_seed(9)
    M, K = 2000, 80
    x = torch.randint(0, 16, (M, 32), generator=gen).float() / 15.0
    x[:, 0] = 1.0
    w = torch.full((K, 32), 5.0).to(BF16)
    inp = SimpleNamespace(x=x.to(BF16), wq=w, bias=None)
    xd, wd = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda")
    e = torch.empty(0, device="cuda")
    cell = ops.reference.xbar_cell_params(1.0, 0.0, xd.device)
    out, _ = ops.ext().xbar_cells_fwd_linear(xd, wd, e.to(BF16), 1, f, 32, 0,
                                             e, 4, 2, cell, 77, False)
    ref = xco.linear_blocked(inp.x, inp.wq, None, "abs", 32, 0, 0.0, 1.0, 0.0,
                             4, 2)
    assert ref.nblocks == 1 and ref.T == 2
    assert float((ref.s[0] - ref.s[1]).abs().max()) == 0.0
    var = xco.noise_variance(ref)
    assert float((var - 17.0 * ref.s[0]).abs().max()) <= 1e-9
    fo.check_noise_field(out, ref.clean, var, FACTOR,
                         stats=("mean", "std", "channel_std"),
                         what="two equal slices")


# ---------------------------------------------------------------------------
# 5. noise and ADC together
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_noise_goes_through_the_adc(shape, dtype, E):
    # integer inputs with w_min 0, so that the offset leaves the step's grid
    # alone; Qu 15 and a power-of-two step sized to the slice partials (about
    # 240 per 64 rows at E = 1, 720 at E = 2, noise sigma about 11 and 19)
    inp = xco.exact_inputs(shape, dtype, w_min=0.0)
    rows, bits = 64, 4
    step = 32.0 if E == 1 else 128.0
    amax = 15 * step
    kw = dict(seed=5, bias=False)
    noisy, _ = _run(shape, inp, "abs", rows, bits, amax, 4, E, 1.0, 0.0, **kw)
    clean, _ = _run(shape, inp, None, rows, bits, amax, 4, E, 1.0, 0.0, **kw)
    o = fo.to_mk(noisy)
    k = o / step
    # shift-adding multiples of a power-of-two step, rounded once to the
    # dtype (an integer count of steps rounds to an integer), stays on the
    # step's grid
    assert torch.equal(k, torch.round(k)), "output off the ADC grid"
    differ = float((o != fo.to_mk(clean)).double().mean())
    print("%s E=%d: %.3f of the outputs moved by the noise" % (shape, E,
                                                               differ))
    assert differ > 0.05


# ---------------------------------------------------------------------------
# 6. seeds
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_seeds(shape):
    inp = xco.general_inputs(shape, BF16, 4)
    cfg = (64, 6, 2.0, 4, 1)
    a, _ = _general(shape, inp, "abs2", *cfg, seed=1001)
    b, _ = _general(shape, inp, "abs2", *cfg, seed=1001)
    c, _ = _general(shape, inp, "abs2", *cfg, seed=1002)
    assert torch.equal(a, b), "same seed, different output"
    assert float((a != c).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# 7. anchor: one slice of unsigned codes is the unsliced kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_slice_of_codes_is_the_unsliced_kernel(shape, dtype):
    # counter ((b*T + t)*M + m)*K + k with T = 1; w_min 0 and w_step 1 make
    # the digit the weight, abs mode makes s = p = sum x * |w_raw|
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = xco.exact_inputs(shape, dtype, w_min=0.0)
    assert torch.equal(inp.wq, inp.code)
    rows = 64
    got, _ = _run(shape, inp, "abs", rows, 0, 0.0, 4, 4, 1.0, 0.0, seed=4242)
    x, wq = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda", dtype=torch.float32)
    e = torch.empty(0, device="cuda", dtype=torch.float32)
    if kind == "conv":
        want, _ = ops.ext().xbar_fwd_conv(x, wq, wq, inp.bias.cuda(), stride,
                                          pad, 1, f, rows, 0, e, 4242, False)
    else:
        want, _ = ops.ext().xbar_fwd_linear(x, wq, wq, inp.bias.cuda(), 1, f,
                                            rows, 0, e, 4242, False)
    assert torch.equal(got, want)
    # and the draw matters: another seed moves the output
    other, _ = _run(shape, inp, "abs", rows, 0, 0.0, 4, 4, 1.0, 0.0,
                    seed=4243)
    assert float((other != want).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# 8. telemetry
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_adc_telemetry_exact(shape):
    inp = xco.exact_inputs(shape, BF16)
    for rows, bits, amax, E in xco.EXACT_CFGS:
        ref = xco.oracle(shape, BF16, "exact", None, rows, bits, amax, 4, E)
        _, tele = _exact(shape, inp, None, rows, bits, amax, E, telem=True)
        assert tele.numel() == 5
        assert float(tele[0]) == 0.0 and float(tele[1]) == 0.0
        assert float(tele[2]) == float(ref.clean.max())
        assert float(tele[3]) == ref.clipped
        assert float(tele[4]) == ref.absmax
    # the public wrapper publishes the share over T * nblocks * M * K
    kind, xs, ws, stride, pad = SHAPES[shape]
    rows, bits, amax, E = xco.EXACT_CFGS[0]
    ref = xco.oracle(shape, BF16, "exact", None, rows, bits, amax, 4, E)
    assert ref.n_partials == 4 * ref.nblocks * ref.out.numel()
    t = ops.XbarTelemetry()
    args = (_dev(inp.x), _dev(inp.wq), _dev(inp.wq), inp.bias.cuda())
    kw = dict(want_telemetry=True, telemetry_out=t, cell_bits=E,
              **xco.EXACT_W)
    if kind == "conv":
        ops.xbar_noisy_conv2d(*args, stride, pad, None, 0.0, rows, bits, amax,
                              **kw)
    else:
        ops.xbar_noisy_linear(*args, None, 0.0, rows, bits, amax, **kw)
    share = xco.clip_share(ref)
    assert abs(float(t.adc_clip_share) - share) <= 2.0 ** -22 * share
    assert float(t.partial_absmax) == ref.absmax
    assert t.power is None and t.nsr is None
    _, none = _exact(shape, inp, None, rows, bits, amax, E, telem=False)
    assert none.numel() == 0


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_noise_telemetry_slots(shape, mode, E):
    # ADC off, general inputs: tele[0] is the cell current, not shift-weighted
    inp = xco.general_inputs(shape, BF16, 4)
    rows = 64
    ref = xco.oracle(shape, BF16, "general", mode, rows, 0, 0.0, 4, E)
    out, tele = _general(shape, inp, mode, rows, 0, 0.0, 4, E, seed=31,
                         telem=True)
    o = fo.to_mk(out)
    rel0 = abs(float(tele[0]) - ref.p_sum) / ref.p_sum
    A = sum(sh * a for sh, a in zip(ref.shift, ref.A)) \
        + abs(ref.w_min) * ref.xabs + ref.bias_abs
    n = ref.n + (ref.T + 1) * ref.nblocks + 2
    s1 = float((o - ref.clean).abs().sum())
    b1 = float((fo.U_OUT[BF16] * o.abs() + fo.gamma(n) * A).sum())
    bm = float(fo.det_bound(ref.clean, A, n, BF16).max())
    e1 = abs(float(tele[1]) - s1)
    e2 = abs(float(tele[2]) - float(ref.clean.max()))
    print("%s %s E=%d: tele0 rel %.3g, tele1 %.3g, tele2 %.3g of bound"
          % (shape, mode, E, rel0, e1 / b1, e2 / bm))
    assert rel0 <= TELE0_REL
    assert e1 <= b1 and e2 <= bm
    assert float(tele[3]) == 0.0
    # max |v_bt| includes the noise: within 6 sigma of the largest partial
    smax = float(max((FACTOR * s).sqrt().max() for s in ref.s))
    assert ref.absmax - 6 * smax <= float(tele[4]) <= ref.absmax + 6 * smax


# ---------------------------------------------------------------------------
# 9. backward and capture
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_is_the_plain_ops(shape):
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = xco.general_inputs(shape, BF16, 4)

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

    kw = dict(cell_bits=1, **xco.general_w(4))
    if kind == "conv":
        got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
            x, w, w.detach(), b, stride, pad, "abs", FACTOR, 64, 4, 1.0, **kw))
        want = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    else:
        got = grads(lambda x, w, b: ops.xbar_noisy_linear(
            x, w, w.detach(), b, "abs", FACTOR, 64, 4, 1.0, **kw))
        want = grads(lambda x, w, b: ops.linear(x, w, b))
    for name, a, b in zip(("gx", "gw", "gb"), got, want):
        assert torch.equal(a, b), name


def test_double_backward_runs():
    kind, xs, ws, stride, pad = SHAPES["convB"]
    inp = xco.general_inputs("convB", FP32, 4)
    x = _dev(inp.x).requires_grad_()
    w = _dev(inp.wq).requires_grad_()
    y = ops.xbar_noisy_conv2d(x, w, w.detach(), None, stride, pad, "abs",
                              FACTOR, 64, 4, 2.0, cell_bits=2,
                              **xco.general_w(4))
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    gx.square().sum().backward()
    assert w.grad is not None and torch.isfinite(w.grad).all()


def test_captured_call_draws_fresh_noise():
    from noisynet_amd.graphs import GraphedTrainStep
    inp = xco.general_inputs("linear", BF16, 4)
    x, w = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda")
    torch.manual_seed(2)

    def body():
        return ops.xbar_noisy_linear(x, w, w, None, "abs", f, 64, 6, 2.0,
                                     cell_bits=1, **xco.general_w(4))

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
    inp = xco.general_inputs(shape, BF16, 4)
    ws, wm = 1.0 / 15.0, -0.5

    def run(mode="abs", rows=64, bits=4, w_bits=4, cell_bits=2):
        return _run(shape, inp, mode, rows, bits, 1.0, w_bits, cell_bits, ws,
                    wm)

    with pytest.raises(RuntimeError, match="cell_bits"):
        run(cell_bits=0)
    with pytest.raises(RuntimeError, match="cell_bits"):
        run(cell_bits=5)
    with pytest.raises(RuntimeError, match="w_bits"):
        run(w_bits=0)
    with pytest.raises(RuntimeError, match="w_bits"):
        run(w_bits=9, cell_bits=3)
    with pytest.raises(RuntimeError, match=r"7 slices.*smallest.*is 2"):
        run(w_bits=7, cell_bits=1)
    with pytest.raises(RuntimeError, match="xbar_rows"):
        run(rows=48)
    with pytest.raises(RuntimeError, match="both off"):
        run(mode=None, bits=0)
    x, w = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda")
    e = torch.empty(0, device="cuda")
    adc = ops.reference.xbar_adc_params(4, 1.0, x.device, unipolar=True)
    with pytest.raises(RuntimeError, match=r"cell must be"):
        bad = ops.reference.xbar_dac_params(ws, x.device)     # two elements
        if x.dim() == 4:
            ops.ext().xbar_cells_fwd_conv(x, w, e.to(BF16), 2, 2, 1, f, 64, 4,
                                          adc, 4, 2, bad, 1, False)
        else:
            ops.ext().xbar_cells_fwd_linear(x, w, e.to(BF16), 1, f, 64, 4,
                                            adc, 4, 2, bad, 1, False)
    out, _ = _run(shape, xco.general_inputs(shape, FP32, 8), "abs", 64, 4,
                  1.0, 8, 2, 1.0 / 255.0, -0.5)
    assert torch.isfinite(out).all()
    for kw in (dict(differential=True),
               dict(in_bits=4, dac_bits=1, x_step=1.0 / 15.0)):
        with pytest.raises(ValueError, match="accumulator sets"):
            if x.dim() == 4:
                ops.xbar_noisy_conv2d(x, w, w, None, 2, 2, "abs", 0.5, 64, 4,
                                      1.0, w_bits=4, cell_bits=2, w_step=ws,
                                      w_min=wm, **kw)
            else:
                ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 1.0,
                                      w_bits=4, cell_bits=2, w_step=ws,
                                      w_min=wm, **kw)


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


def test_model_trains_a_step_on_bit_sliced_weights():
    base = ['--xbar_rows', '128', '--xbar_cell_bits', '2', '--q_w', '4']
    x, y = _batch()
    # the per-slice, unipolar range is read off the printed max: one forward
    # with the ADC off collects max|partial| per layer
    probe = _model(base)
    probe.train()
    with torch.no_grad():
        probe(x, 0, 0)
    amax = [probe.partial_absmax[k][0] for k in range(4)]
    print("per-slice max |partial| of the four layers:",
          ", ".join("%.3g" % a for a in amax))
    assert all(a > 0 for a in amax)
    extra = ['--q_adc', '6']
    for k, a in enumerate(amax):
        extra += ['--adc_max%d' % (k + 1), repr(a)]
    model = _model(base + extra)
    model.train()
    loss = ops.cross_entropy(model(x, 0, 0), y)
    loss.backward()
    assert torch.isfinite(loss)
    for name in ('conv1', 'conv2', 'linear1', 'linear2'):
        g = getattr(model, name).weight.grad
        assert g is not None and torch.isfinite(g.float()).all(), name
    for k in range(4):
        assert len(model.adc_clip[k]) == 1
        assert 0.0 <= model.adc_clip[k][0] <= 0.5
        assert model.partial_absmax[k][0] > 0
        assert len(model.power[k]) == 1
