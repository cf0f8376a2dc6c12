"""ops.bn_act_quant (csrc/bn_act_quant.hip) against the composition it fuses.

The fused forward replaces bn_act -> fake_quant -> max() -> pad_cols8; the
backward runs the composition's kernels on the activation the fused forward
stored. The contract is bit-identity, so every comparison is torch.equal
against that composition built from the existing ops, with torch.manual_seed
set to the same value before each side (the stochastic-rounding seed is drawn
from torch's generator). Tensors with numel % 4 != 0 are handed to the
composition by ops.bn_act_quant itself (see bn_act_quant_native); those shapes
stay in the matrix and check that hand-over.
"""

import os

import pytest
import torch
import torch.nn.functional as F

from noisynet_amd import ops, utils
from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser
from noisynet_amd.models.noisynet import Net
from noisynet_amd.quant import finish_calibration, start_calibration

pytestmark = pytest.mark.gpu

MOMENTUM, EPS, BITS = 0.1, 1e-5, 4

# (N, C, H, W)
SHAPES = [
    (3, 65, 14, 14),    # Philox quads straddle pixels, 7 pad channels
    (2, 5, 7, 7),       # numel % 4 != 0: handed to the composition
    (4, 5, 7, 7),       # C < 8, pad 3
    (2, 64, 6, 6),      # no padding
    (2, 72, 4, 4),      # no padding
    (1, 1, 3, 3),       # numel % 4 != 0
    (4, 1, 3, 3),
    (700, 65, 14, 14),  # past the forward grid cap: the slab-stride loop
]
# backward only: odd row counts and a 2-D input
BWD_SHAPES = [(4, 65, 5, 3), (4, 13, 5, 5), (36, 21)]
DTYPES = [torch.bfloat16, torch.float16]
# (act_max, max_value, whether an activation can reach the top code).
# act_max 0.7 rounds DOWN in bf16 (0.69921875); max_value sits below, at and
# above the clip (with no clip: inside and above the value range).
ACT_AND_QMAX = [(0.0, 1.5, True), (0.0, 3.0, True), (0.0, 40.0, False),
                (0.7, 0.5, True), (0.7, 0.7, True), (0.7, 1.0, False),
                (5.0, 3.0, True), (5.0, 5.0, True), (5.0, 6.0, False)]


def _round8(c):
    return (c + 7) // 8 * 8


def _inputs(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = (torch.randn(shape, generator=g) * 2.0 + 0.3).to(dtype).cuda()
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    # gamma up to 3 and beta up to 1: the normalised values reach past 5
    weight = (0.5 + 2.5 * torch.rand(C, generator=g)).cuda()
    bias = (-0.5 + 1.5 * torch.rand(C, generator=g)).cuda()
    rmean = torch.randn(C, generator=g).cuda()
    rvar = (0.5 + torch.rand(C, generator=g)).cuda()
    gout = torch.randn(shape, generator=g).to(dtype).cuda()
    if len(shape) == 4:
        gout = gout.contiguous(memory_format=torch.channels_last)
    return x, weight, bias, rmean, rvar, gout


def _rows(t):
    """[rows, C] NHWC rows of a 4-D (or 2-D) tensor."""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t


def _composition(x, weight, bias, rmean, rvar, gout, act_max, qmax, stoch,
                 seed=11):
    x = x.clone().requires_grad_(True)
    weight = weight.clone().requires_grad_(True)
    bias = bias.clone().requires_grad_(True)
    rmean, rvar = rmean.clone(), rvar.clone()
    torch.manual_seed(seed)
    a = ops.bn_act(x, weight, bias, rmean, rvar, True, MOMENTUM, EPS,
                   relu=True, act_max=act_max)
    q = ops.fake_quant(a, BITS, 0.0, qmax, stoch)
    q.backward(gout)
    return dict(a=a.detach(), q=q.detach(), max=q.detach().max(),
                gx=x.grad, gw=weight.grad, gb=bias.grad, rmean=rmean,
                rvar=rvar)


def _fused(x, weight, bias, rmean, rvar, gout, act_max, qmax, stoch, c_pad,
           seed=11):
    x = x.clone().requires_grad_(True)
    weight = weight.clone().requires_grad_(True)
    bias = bias.clone().requires_grad_(True)
    rmean, rvar = rmean.clone(), rvar.clone()
    torch.manual_seed(seed)
    xq, x_pad, xmax = ops.bn_act_quant(x, weight, bias, rmean, rvar, MOMENTUM,
                                       EPS, act_max, BITS, 0.0, qmax, stoch,
                                       c_pad=c_pad)
    xq.backward(gout)
    return dict(xq=xq.detach(), x_pad=x_pad, max=xmax, gx=x.grad,
                gw=weight.grad, gb=bias.grad, rmean=rmean, rvar=rvar)


def _check(shape, dtype, act_max, qmax, stoch, c_pad, assert_sets=True,
           top_reachable=True):
    inp = _inputs(shape, dtype)
    ref = _composition(*inp, act_max, qmax, stoch)
    out = _fused(*inp, act_max, qmax, stoch, c_pad)
    C = shape[1]

    if assert_sets and inp[0].numel() >= 1000:
        # the inputs exercise every branch: relu zeros, the clip, the
        # quantiser's top code (reachable when the range ends at or below
        # the largest activation)
        a = ref['a'].float()
        assert (a == 0).any()
        if act_max > 0:
            thr = torch.tensor(act_max).to(dtype).float().item()
            assert (a == thr).any()
        if top_reachable:
            top = torch.tensor(qmax).to(dtype).float().item()
            assert (ref['q'].float() == top).any()

    # forward: the logical tensor, the padded buffer, the maximum
    assert out['xq'].shape == ref['q'].shape
    assert torch.equal(out['xq'], ref['q'])
    native = ops.bn_act_quant_native(inp[0], inp[3], 0.0)
    assert native == (inp[0].numel() % 4 == 0)
    if c_pad == C or not native:
        assert out['x_pad'] is None
    else:
        want = F.pad(_rows(ref['q']), (0, c_pad - C))
        assert out['x_pad'].shape == want.shape
        assert out['x_pad'].is_contiguous()
        assert torch.equal(out['x_pad'], want)
        assert (out['x_pad'][:, C:] == 0).all()
    assert out['max'].dtype == ref['max'].dtype
    assert out['max'].shape == ref['max'].shape
    assert torch.equal(out['max'], ref['max'])
    assert torch.equal(out['rmean'], ref['rmean'])
    assert torch.equal(out['rvar'], ref['rvar'])
    # backward
    assert torch.equal(out['gx'], ref['gx'])
    assert torch.equal(out['gw'], ref['gw'])
    assert torch.equal(out['gb'], ref['gb'])


@pytest.mark.parametrize("stoch", [0.5, 0.0])
@pytest.mark.parametrize("act_max,qmax,top", ACT_AND_QMAX)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_composition(shape, dtype, act_max, qmax, top, stoch):
    C = shape[1]
    _check(shape, dtype, act_max, qmax, stoch, _round8(C), top_reachable=top)


@pytest.mark.parametrize("shape", [(3, 65, 14, 14), (4, 5, 7, 7)],
                         ids=lambda s: "x".join(map(str, s)))
def test_unpadded_odd_channels(shape):
    """C_pad == C with C % 8 != 0: no padded buffer, values written in place."""
    _check(shape, torch.bfloat16, 5.0, 3.0, 0.5, shape[1])


@pytest.mark.parametrize("stoch", [0.5, 0.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", BWD_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_backward_tails(shape, dtype, stoch):
    for act_max, qmax in [(0.7, 0.7), (5.0, 3.0)]:
        _check(shape, dtype, act_max, qmax, stoch, _round8(shape[1]),
               assert_sets=False)


def test_conv_takes_the_padded_tensor():
    """fused_noisy_conv2d on (view, x_pad) equals the conv of the composition's
    quantised tensor, forward and backward, with the max as input_max."""
    shape, dtype = (4, 65, 14, 14), torch.bfloat16
    x, weight, bias, rmean, rvar, _ = _inputs(shape, dtype)
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(120, 65, 5, 5, generator=g) * 0.05).to(dtype).cuda()
    w = w.contiguous(memory_format=torch.channels_last)
    assert ops.conv_input_pad_width(x, w) == 72

    def run(fused):
        xx = x.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        gam = weight.clone().requires_grad_(True)
        bet = bias.clone().requires_grad_(True)
        torch.manual_seed(21)
        if fused:
            xq, x_pad, xmax = ops.bn_act_quant(
                xx, gam, bet, rmean.clone(), rvar.clone(), MOMENTUM, EPS, 5.0,
                BITS, 0.0, 3.0, 0.5, c_pad=72)
            assert x_pad is not None
        else:
            a = ops.bn_act(xx, gam, bet, rmean.clone(), rvar.clone(), True,
                           MOMENTUM, EPS, relu=True, act_max=5.0)
            xq = ops.fake_quant(a, BITS, 0.0, 3.0, 0.5)
            x_pad, xmax = None, xq.detach().max()
        factor = 0.1 * xmax / 1.0
        y = ops.fused_noisy_conv2d(xq, ww, ww.detach(), None, 1, 0, 'abs2',
                                   factor, current=1.0, power_denom=xmax,
                                   x_pad=x_pad)
        y.float().square().sum().backward()
        return y.detach(), xx.grad, ww.grad, gam.grad, bet.grad

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def _flagship(batch=8, seed=3):
    argv = ["--current", "1", "--q_a", "4", "--act_max", "5", "--w_max1",
            "0.3", "--LR", "0.005", "--L2_1", "0.0005", "--L2_2", "0.0002",
            "--batch_size", str(batch), "--calculate_running"]
    args = build_noisynet_parser().parse_args(argv)
    broadcast_per_layer(args)
    torch.manual_seed(seed)
    model = Net(args)
    utils.init_model(model, args)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.float()
    return model.to(memory_format=torch.channels_last)


def _model_step(no_fuse):
    old = os.environ.pop("NOISYNET_NO_BN_QUANT_FUSE", None)
    if no_fuse:
        os.environ["NOISYNET_NO_BN_QUANT_FUSE"] = "1"
    try:
        model = _flagship()
        g = torch.Generator().manual_seed(9)
        x = (torch.randint(0, 16, (8, 3, 32, 32), generator=g).cuda()
             .bfloat16() / 15.0).contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 10, (8,), generator=g).cuda()
        start_calibration(model)
        with torch.no_grad():
            for i in range(5):
                model(x, 0, i)
        finish_calibration(model, torch.device("cuda"))
        model.train()
        torch.manual_seed(17)
        taken = []
        orig = ops.bn_act_quant

        def spy(*a, **k):
            taken.append(1)
            return orig(*a, **k)

        ops.bn_act_quant = spy
        try:
            out = model(x, 0, 100)
        finally:
            ops.bn_act_quant = orig
        loss = ops.cross_entropy(out, y)
        loss.backward()
        torch.cuda.synchronize()
        return dict(
            taken=bool(taken), out=out.detach(),
            grads={n: p.grad for n, p in model.named_parameters()},
            bufs={n: b.detach().clone() for n, b in model.named_buffers()},
            last_range=model.quantize2.last_range)
    finally:
        os.environ.pop("NOISYNET_NO_BN_QUANT_FUSE", None)
        if old is not None:
            os.environ["NOISYNET_NO_BN_QUANT_FUSE"] = old


def test_model_step_matches_composition():
    fused, comp = _model_step(False), _model_step(True)
    assert fused['taken'] and not comp['taken']
    assert torch.equal(fused['out'], comp['out'])
    assert fused['grads'].keys() == comp['grads'].keys()
    for n in fused['grads']:
        assert fused['grads'][n] is not None, n
        assert torch.equal(fused['grads'][n], comp['grads'][n]), n
    for n in fused['bufs']:
        assert torch.equal(fused['bufs'][n], comp['bufs'][n]), n
    assert fused['last_range'] == comp['last_range']
    assert fused['last_range'] is not None and fused['last_range'][0] == 0


def test_graph_capture_and_replay():
    """One capture + replay of the fused op (forward and backward) equals the
    eager call under the same live step counter."""
    shape, dtype = (3, 65, 14, 14), torch.bfloat16
    x, weight, bias, rmean, rvar, gout = _inputs(shape, dtype)
    seed_buf = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    ops.ext().set_seed_buffer(seed_buf)
    try:
        xs = x.clone().requires_grad_(True)
        ws = weight.clone().requires_grad_(True)
        bs = bias.clone().requires_grad_(True)

        def body():
            xs.grad = ws.grad = bs.grad = None
            xq, x_pad, xmax = ops.bn_act_quant(
                xs, ws, bs, None, None, MOMENTUM, EPS, 5.0, BITS, 0.0, 3.0,
                0.5, c_pad=72)
            xq.backward(gout)
            return x_pad, xmax, xs.grad, ws.grad, bs.grad

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.manual_seed(31)
            eager = [t.clone() for t in body()]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

        graph = torch.cuda.CUDAGraph()
        torch.manual_seed(31)
        with torch.cuda.graph(graph):
            captured = body()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
        # the draws follow the live counter: another value, other roundings
        seed_buf.add_(1)
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.equal(eager[0], captured[0])
    finally:
        ops.ext().clear_seed_buffer()
