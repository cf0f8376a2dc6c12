"""The fused tiled-crossbar kernel (per-block noise + ADC) against the fp64
oracle of xbar_oracle.py.

Shapes are the smallest that still cross every boundary of the 64x64x32 tile:
  linear   M=130 (three ragged m-tiles, M % 4 != 0), Kc=296 (tail k-step; the
           last block is short for 128/64/32 rows), K=80 (two ragged n-tiles)
  conv A   x [3,5,9,9], w [70,5,5,5], stride 2, pad 2: odd C, n=125, spans
           that straddle filter taps, padding rows
  conv B   x [3,32,6,6], w [20,32,3,3], stride 1, pad 1: C % 32 == 0, the
           16-byte activation staging path
"""

import os
import sys
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
import xbar_oracle as xo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
MODE_INT = {None: 0, "abs": 1, "abs2": 2}
FACTOR = 0.5
# relative error allowed on the float-atomic sum of sigma_abs: the bound of
# tests/test_fused_noise_gpu.py (TELE0_REL), whose reasoning applies unchanged
TELE0_REL = 2.8e-6

# name -> (kind, x shape, w shape, stride, pad)
SHAPES = {
    "linear": ("linear", (130, 296), (80, 296), 1, 0),
    "convA": ("conv", (3, 5, 9, 9), (70, 5, 5, 5), 2, 2),
    "convB": ("conv", (3, 32, 6, 6), (20, 32, 3, 3), 1, 1),
}
EXACT_CFGS = [(128, 4, 112.0), (64, 4, 56.0), (32, 6, 62.0)]
GENERAL_CFGS = {
    "linear": [(128, 6, 3.0), (64, 4, 2.0), (32, 8, 1.5)],
    "convA": [(64, 5, 1.5), (32, 4, 1.0)],
}


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _dev(t):
    t = t.cuda()
    if t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t


@lru_cache(maxsize=None)
def _general_inputs(shape, dtype, seed=1, batch=None):
    kind, xs, ws, stride, pad = SHAPES[shape]
    if batch is not None:
        xs = (batch,) + xs[1:]
    return fo.make_inputs(xs, ws, dtype, seed)


@lru_cache(maxsize=None)
def _exact_inputs(shape, dtype):
    """Integer-grid inputs: x = randint(0,16), wq = randint(-8,9)/8, bias a
    multiple of 1/8. With a power-of-two step every product, partial sum and
    v/step is exact in fp32 in any order."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    gen = torch.Generator().manual_seed(17)
    return SimpleNamespace(
        x=torch.randint(0, 16, xs, generator=gen).float().to(dtype),
        wq=(torch.randint(-8, 9, ws, generator=gen).float() / 8).to(dtype),
        w_raw=(torch.randint(-8, 9, ws, generator=gen).float() / 8).to(dtype),
        bias=(torch.randint(-8, 9, (ws[0],), generator=gen).float() / 8).to(dtype))


@lru_cache(maxsize=None)
def _oracle(shape, dtype, inputs, mode, rows, bits, amax, bias=True,
            batch=None):
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = _exact_inputs(shape, dtype) if inputs == "exact" \
        else _general_inputs(shape, dtype, batch=batch)
    b = inp.bias if bias else None
    if kind == "conv":
        return xo.conv_blocked(inp.x, inp.wq, inp.w_raw, b, stride, pad, mode,
                               rows, bits, amax)
    return xo.linear_blocked(inp.x, inp.wq, inp.w_raw, b, mode, rows, bits,
                             amax)


def _run(shape, inp, mode, rows, bits, amax, seed=1, telem=False, bias=True,
         factor=FACTOR, mode_int=None):
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
    mi = MODE_INT[mode] if mode_int is None else mode_int
    if kind == "conv":
        out, tele = ops.ext().xbar_fwd_conv(x, wq, wr, b, stride, pad, mi, f,
                                            rows, bits, adc, seed, telem)
    else:
        out, tele = ops.ext().xbar_fwd_linear(x, wq, wr, b, mi, f, rows, bits,
                                              adc, seed, telem)
    return out, tele.double().cpu()


# ---------------------------------------------------------------------------
# 1. exact: noise off, ADC on, power-of-two step
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_adc(shape, dtype):
    inp = _exact_inputs(shape, dtype)
    for rows, bits, amax in EXACT_CFGS:
        ref = _oracle(shape, dtype, "exact", None, rows, bits, amax)
        out, _ = _run(shape, inp, None, rows, bits, amax)
        assert out.dtype == dtype
        want = ref.out.to(dtype)          # fp32-exact, rounded once
        got = fo.to_mk(out).to(dtype)
        clip = ref.clipped / float(ref.nblocks * ref.out.numel())
        ties = sum(float(((t - torch.floor(t)) == 0.5).double().mean())
                   for t in ref.t) / ref.nblocks
        print("%s %s rows %d: clip share %.3f, tie share %.4f, mismatches %d"
              % (shape, _name(dtype), rows, clip, ties,
                 int((got != want).sum())))
        assert torch.equal(got, want)


def test_exact_inputs_exercise_clipping_and_ties():
    ref = _oracle("linear", FP32, "exact", None, 64, 4, 56.0)
    clip = ref.clipped / float(ref.nblocks * ref.out.numel())
    ties = sum(float(((t - torch.floor(t)) == 0.5).double().mean())
               for t in ref.t) / ref.nblocks
    assert clip > 0.01 and ties > 0.002, (clip, ties)


# ---------------------------------------------------------------------------
# 2. general inputs: noise off, ADC on
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", list(GENERAL_CFGS))
def test_general_adc(shape, dtype):
    inp = _general_inputs(shape, dtype)
    for rows, bits, amax in GENERAL_CFGS[shape]:
        ref = _oracle(shape, dtype, "general", None, rows, bits, amax)
        for bias in (True, False):
            if not bias:
                ref = _oracle(shape, dtype, "general", None, rows, bits, amax,
                              False)
            for telem in (False, True):
                out, _ = _run(shape, inp, None, rows, bits, amax, telem=telem,
                              bias=bias)
                xo.assert_adc_close(out, ref, rows, dtype, "%s %s %s b%d t%d"
                                    % (shape, _name(dtype),
                                       (rows, bits, amax), bias, telem))


@pytest.mark.parametrize("shape", ["linear", "convA", "convB"])
def test_one_block(shape):
    # xbar_rows >= n: one block; with the ADC on it is the ADC of the plain op
    inp = _general_inputs(shape, BF16)
    ref = _oracle(shape, BF16, "general", None, 1024, 5, 4.0)
    assert ref.nblocks == 1
    out, _ = _run(shape, inp, None, 1024, 5, 4.0)
    xo.assert_adc_close(out, ref, ref.n, BF16, shape + " one block")
    # and with both noise and ADC off there is nothing to run
    with pytest.raises(RuntimeError, match="both off"):
        _run(shape, inp, None, 1024, 0, 0.0)
    kind, xs, ws, stride, pad = SHAPES[shape]
    with pytest.raises(ValueError, match="neither"):
        if kind == "conv":
            ops.xbar_noisy_conv2d(_dev(inp.x), _dev(inp.wq), _dev(inp.w_raw),
                                  None, stride, pad, None, 0.0, 1024, 0, 0.0)
        else:
            ops.xbar_noisy_linear(_dev(inp.x), _dev(inp.wq), _dev(inp.w_raw),
                                  None, None, 0.0, 1024, 0, 0.0)


# ---------------------------------------------------------------------------
# 3. ADC off, noise on: blocking alone changes nothing statistically
# ---------------------------------------------------------------------------

NOISE_BATCH = {"linear": 1700, "convB": 200}      # >= 2^17 outputs each


@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape,rows", [("linear", 64), ("convB", 32),
                                        ("convB", 128)])
def test_noise_field_blocked(shape, rows, mode):
    batch = NOISE_BATCH[shape]
    inp = _general_inputs(shape, BF16, batch=batch)
    ref = _oracle(shape, BF16, "general", mode, rows, 0, 0.0, True, batch)
    assert ref.out.numel() >= 1 << 17 and ref.nblocks >= 3
    out, _ = _run(shape, inp, mode, rows, 0, 0.0, seed=1234)
    fo.check_noise_field(out, ref.clean, sum(ref.s), FACTOR,
                         what="%s rows %d %s" % (shape, rows, mode))


def test_block_draws_are_independent():
    # three equal blocks: independent draws give variance factor * 3 s_0,
    # one draw reused for every block would give 3x that
    gen = torch.Generator().manual_seed(9)
    M, K = 2000, 80
    xb = (torch.randint(1, 16, (M, 32), generator=gen).float() / 15).to(BF16)
    wb = (torch.randn(K, 32, generator=gen) * 0.05).to(BF16)
    inp = SimpleNamespace(x=xb.repeat(1, 3), wq=wb.repeat(1, 3),
                          w_raw=wb.repeat(1, 3), bias=None)
    x, w = _dev(inp.x), _dev(inp.wq)
    f = torch.tensor([FACTOR], device="cuda")
    e = torch.empty(0, device="cuda")
    out, _ = ops.ext().xbar_fwd_linear(x, w, w, e.to(BF16), 1, f, 32, 0, e,
                                       77, False)
    ref = xo.linear_blocked(inp.x, inp.wq, inp.w_raw, None, "abs", 32, 0, 0.0)
    assert ref.nblocks == 3
    assert float((ref.s[0] - ref.s[2]).abs().max()) == 0.0
    fo.check_noise_field(out, ref.clean, sum(ref.s), FACTOR,
                         stats=("mean", "std", "channel_std"),
                         what="three equal blocks")


# ---------------------------------------------------------------------------
# 4. noise and ADC together
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_noise_goes_through_the_adc(shape, dtype):
    inp = _general_inputs(shape, dtype)
    rows, bits, amax = 64, 4, 1.75                # Qm 7 -> step 0.25
    ref = _oracle(shape, dtype, "general", "abs", rows, bits, amax, False)
    assert ref.step == 0.25
    noisy, _ = _run(shape, inp, "abs", rows, bits, amax, seed=5, bias=False)
    clean, _ = _run(shape, inp, None, rows, bits, amax, seed=5, bias=False)
    o = fo.to_mk(noisy)
    k = o / ref.step
    assert torch.equal(k, torch.round(k)), "output off the ADC grid"
    assert float(o.abs().max()) <= ref.nblocks * amax
    differ = float((o != fo.to_mk(clean)).double().mean())
    print("%s: %.3f of the outputs moved by the noise" % (shape, differ))
    assert differ > 0.05


# ---------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_seeds(shape):
    inp = _general_inputs(shape, BF16)
    a, _ = _run(shape, inp, "abs2", 64, 6, 3.0, seed=1001)
    b, _ = _run(shape, inp, "abs2", 64, 6, 3.0, seed=1001)
    c, _ = _run(shape, inp, "abs2", 64, 6, 3.0, seed=1002)
    assert torch.equal(a, b), "same seed, different output"
    assert float((a != c).double().mean()) > 0.05


def test_block_zero_draws_what_the_unblocked_kernel_draws():
    # counter (b*M + m)*K + k: one block, ADC off, no bias is the unblocked
    # fused linear (same tile, same k-step order) under the same seed
    inp = _general_inputs("linear", BF16)
    x, wq, wr = _dev(inp.x), _dev(inp.wq), _dev(inp.w_raw)
    assert ops.ext().linear_fused_route(296, 80, 2) == "gemm"
    f = torch.tensor([FACTOR], device="cuda", dtype=torch.float32)
    e = torch.empty(0, device="cuda", dtype=BF16)
    want = ops.ext().linear_fwd_fused(x, wq, wr, e, 1, f, 4242, False)[0]
    got, _ = _run("linear", inp, "abs", 1024, 0, 0.0, seed=4242, bias=False)
    assert torch.equal(got, want)
    # with three blocks the first block's draw is still that one, the sum is not
    got3, _ = _run("linear", inp, "abs", 128, 0, 0.0, seed=4242, bias=False)
    assert float((got3 != want).double().mean()) > 0.5


# ---------------------------------------------------------------------------
# telemetry
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_adc_telemetry_exact(shape):
    inp = _exact_inputs(shape, BF16)
    for rows, bits, amax in EXACT_CFGS:
        ref = _oracle(shape, BF16, "exact", None, rows, bits, amax)
        _, tele = _run(shape, inp, None, rows, bits, amax, telem=True)
        assert tele.numel() == 5
        assert float(tele[0]) == 0.0 and float(tele[1]) == 0.0
        assert float(tele[2]) == float(ref.clean.max())
        assert float(tele[3]) == ref.clipped
        assert float(tele[4]) == ref.absmax
    # the public wrapper publishes the share and the maximum
    kind, xs, ws, stride, pad = SHAPES[shape]
    rows, bits, amax = EXACT_CFGS[1]
    ref = _oracle(shape, BF16, "exact", None, rows, bits, amax)
    t = ops.XbarTelemetry()
    args = (_dev(inp.x), _dev(inp.wq), _dev(inp.w_raw), inp.bias.cuda())
    if kind == "conv":
        ops.xbar_noisy_conv2d(*args, stride, pad, None, 0.0, rows, bits, amax,
                              want_telemetry=True, telemetry_out=t)
    else:
        ops.xbar_noisy_linear(*args, None, 0.0, rows, bits, amax,
                              want_telemetry=True, telemetry_out=t)
    share = ref.clipped / float(ref.nblocks * ref.out.numel())
    assert abs(float(t.adc_clip_share) - share) <= 2.0 ** -22 * share
    assert float(t.partial_absmax) == ref.absmax
    assert t.power is None and t.nsr is None
    _, none = _run(shape, inp, None, rows, bits, amax, telem=False)
    assert none.numel() == 0


@pytest.mark.parametrize("mode", ["abs", "abs2"])
@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_legacy_telemetry_slots(shape, mode):
    # ADC off: the three slots mean what they mean in the unblocked kernels
    inp = _general_inputs(shape, BF16)
    rows = 64
    ref = _oracle(shape, BF16, "general", mode, rows, 0, 0.0)
    out, tele = _run(shape, inp, mode, rows, 0, 0.0, seed=31, telem=True)
    o = fo.to_mk(out)
    A = sum(ref.A) + ref.bias_abs
    n = ref.n + ref.nblocks
    s_abs = float(sum(ref.s_abs).sum())
    rel0 = abs(float(tele[0]) - s_abs) / s_abs
    s1 = float((o - ref.clean).abs().sum())
    b1 = float((fo.U_OUT[BF16] * o.abs() + fo.gamma(n) * A).sum())
    bm = float(fo.det_bound(ref.clean, A, n, BF16).max())
    e1 = abs(float(tele[1]) - s1)
    e2 = abs(float(tele[2]) - float(ref.clean.max()))
    print("%s %s: tele0 rel %.3g, tele1 %.3g, tele2 %.3g of bound"
          % (shape, mode, rel0, e1 / b1, e2 / bm))
    assert rel0 <= TELE0_REL
    assert e1 <= b1 and e2 <= bm
    assert float(tele[3]) == 0.0
    # max |v_b| includes the noise: at least the largest clean partial's
    # neighbourhood, at most that plus 6 sigma
    smax = float(max((FACTOR * s).sqrt().max() for s in ref.s))
    assert ref.absmax - 6 * smax <= float(tele[4]) <= ref.absmax + 6 * smax


# ---------------------------------------------------------------------------
# argument validation in the C++ entry points
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["linear", "convA"])
def test_cpp_argument_validation(shape):
    inp = _general_inputs(shape, BF16)
    with pytest.raises(RuntimeError, match="xbar_rows"):
        _run(shape, inp, "abs", 48, 4, 1.0)
    with pytest.raises(RuntimeError, match="xbar_rows"):
        _run(shape, inp, "abs", 0, 4, 1.0)
    with pytest.raises(RuntimeError, match="adc_bits"):
        _run(shape, inp, "abs", 64, 1, 1.0)
    with pytest.raises(RuntimeError, match="adc_bits"):
        _run(shape, inp, "abs", 64, 17, 1.0)
    with pytest.raises(RuntimeError, match="sigma_mode"):
        _run(shape, inp, None, 64, 4, 1.0, mode_int=3)
    with pytest.raises(RuntimeError, match="sigma_mode"):
        _run(shape, inp, None, 64, 4, 1.0, mode_int=-1)
    x, w = _dev(inp.x), _dev(inp.wq)
    with pytest.raises(ValueError, match="adc_max"):
        if x.dim() == 4:
            ops.xbar_noisy_conv2d(x, w, w, None, 2, 2, "abs", 0.5, 64, 4, 0.0)
        else:
            ops.xbar_noisy_linear(x, w, w, None, "abs", 0.5, 64, 4, 0.0)


# ---------------------------------------------------------------------------
# backward: exactly the unblocked op's gradients
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_is_the_plain_ops(shape):
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = _general_inputs(shape, BF16)

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
    if kind == "conv":
        got = grads(lambda x, w, b: ops.xbar_noisy_conv2d(
            x, w, wr, b, stride, pad, "abs", FACTOR, 64, 4, 1.0))
        want = grads(lambda x, w, b: ops.conv2d(x, w, b, stride, pad))
    else:
        got = grads(lambda x, w, b: ops.xbar_noisy_linear(
            x, w, wr, b, "abs", FACTOR, 64, 4, 1.0))
        want = grads(lambda x, w, b: ops.linear(x, w, b))
    for name, a, b in zip(("gx", "gw", "gb"), got, want):
        assert torch.equal(a, b), name


def test_double_backward_runs():
    kind, xs, ws, stride, pad = SHAPES["convB"]
    inp = _general_inputs("convB", FP32)
    x = _dev(inp.x).requires_grad_()
    w = _dev(inp.wq).requires_grad_()
    y = ops.xbar_noisy_conv2d(x, w, _dev(inp.w_raw), None, stride, pad, "abs",
                              FACTOR, 64, 4, 1.0)
    (gx,) = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    gx.square().sum().backward()
    assert w.grad is not None and torch.isfinite(w.grad).all()


# ---------------------------------------------------------------------------
# graph capture: every replay draws fresh noise
# ---------------------------------------------------------------------------


def test_captured_call_draws_fresh_noise():
    from noisynet_amd.graphs import GraphedTrainStep
    inp = _general_inputs("linear", BF16)
    x, w, wr = _dev(inp.x), _dev(inp.wq), _dev(inp.w_raw)
    f = torch.tensor([FACTOR], device="cuda")
    torch.manual_seed(2)

    def body():
        return ops.xbar_noisy_linear(x, w, wr, None, "abs", f, 64, 6, 3.0)

    gstep = GraphedTrainStep(body, warmup=1)
    first = gstep.replay().clone()
    second = gstep.replay().clone()
    gstep.close()
    torch.cuda.synchronize()
    assert torch.isfinite(first.float()).all()
    assert float((first != second).double().mean()) > 0.05


# ---------------------------------------------------------------------------
# model
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


def test_model_trains_a_step_on_tiled_crossbars():
    model = _model(['--xbar_rows', '128', '--q_adc', '6', '--adc_max', '3'])
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


def test_model_without_tiling_is_todays_path():
    x, _ = _batch()
    outs = []
    for _ in range(2):
        model = _model(['--xbar_rows', '0'], seed=4)
        model.train()
        torch.manual_seed(6)
        outs.append(model(x, 0, 0))
        assert not model.adc_clip[0] and len(model.power[0]) == 1
    assert torch.equal(outs[0], outs[1])
