"""GPU tests of the epilogue kernels against the fp64 oracle
(tests/epilogue_oracle.py): BatchNorm + ReLU + clip (csrc/bn_act.hip),
relu_clip, the activations and SE gating (csrc/activations.hip), the generic
pools (csrc/pool.hip) and softmax cross-entropy (csrc/softmax_xent.hip).

Inputs are drawn on the CPU already rounded to the dtype under test; every
result is moved to the CPU and compared in fp64 with the oracle's derived
bounds (or, for the f32 transcendental activations, 4x the error recorded in
profiles/epilogue_oracle.md). test_epilogue_oracle.py shows on the CPU that
each of these checks can fail.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import epilogue_oracle as eo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOM = 0.1


def dev(t):
    return t.cuda()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 \
        else t.contiguous()


def ext():
    return ops.ext()


def name(dtype):
    return str(dtype).replace("torch.", "")


# ---------------------------------------------------------------------------
# BN + ReLU + clip
# ---------------------------------------------------------------------------


def _bn_stats_check(inp, x, what):
    """bn_stats and bn_stats_finalize (running buffers included) against the
    oracle; returns the kernel's own (mean, invstd) for the later stages."""
    mean_s, var_s = ext().bn_stats(x)
    rm, rv = dev(inp.running_mean.clone()), dev(inp.running_var.clone())
    mean, invstd = ext().bn_stats_finalize(x, rm, rv, MOM, EPS)
    rep = eo.check_stats(mean_s, var_s, None, inp.x, EPS)
    rep.update({"fin_" + k: v for k, v in eo.check_stats(
        mean, None, invstd, inp.x, EPS).items()})
    rep.update(eo.check_running(rm, rv, inp.x, inp.running_mean,
                                inp.running_var, MOM))
    eo.assert_ok(rep, what + " stats")
    # no running buffers: same statistics, bit for bit
    empty = torch.empty(0, device="cuda")
    mean2, invstd2 = ext().bn_stats_finalize(x, empty, empty, MOM, EPS)
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2), what
    return mean, invstd


def _bn_flags_check(inp, x, g, mean, invstd, relu, act_max, dtype, what,
                    autograd=True):
    w, b = dev(inp.weight), dev(inp.bias)
    y = ext().bn_act_fwd(x, mean, invstd, w, b, relu, act_max)
    fwd = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias, relu,
                        act_max, dtype)
    eo.assert_ok(eo.check_act_fwd(y, fwd, relu, act_max, dtype), what + " fwd")
    outs = {}
    for training in (False, True):
        gx, gg, gb = ext().bn_act_bwd(g, x, y, mean, invstd, w, training,
                                      relu, act_max)
        rep, _ = eo.check_bn_bwd(gx, gg, gb, y, fwd, inp.g, training, relu,
                                 act_max, dtype)
        eo.assert_ok(rep, what + (" bwd train" if training else " bwd eval"))
        # the file's stated contract: same inputs, same bits
        again = ext().bn_act_bwd(g, x, y, mean, invstd, w, training, relu,
                                 act_max)
        for a, c in zip((gx, gg, gb), again):
            assert torch.equal(a, c), what + " not bit-identical"
        outs[training] = (gx, gg, gb)
    assert torch.equal(y, ext().bn_act_fwd(x, mean, invstd, w, b, relu,
                                           act_max)), what
    if autograd:
        _bn_autograd_check(inp, x, g, y, mean, invstd, outs, relu, act_max,
                           what)
    return y, fwd


def _bn_autograd_check(inp, x, g, y, mean, invstd, outs, relu, act_max, what):
    """ops.bn_act runs the same kernels: its outputs must equal the direct
    calls bit for bit. Train: the calls checked against the oracle above.
    Eval: direct calls on the running buffers' mean and invstd."""
    for training in (True, False):
        xg = x.clone().requires_grad_(True)
        w = dev(inp.weight).requires_grad_(True)
        b = dev(inp.bias).requires_grad_(True)
        rm, rv = dev(inp.running_mean.clone()), dev(inp.running_var.clone())
        if training:
            y_d, (gx, gg, gb) = y, outs[True]
        else:
            invstd_e = (rv + EPS).rsqrt()
            wd, bd = w.detach(), b.detach()
            y_d = ext().bn_act_fwd(x, rm, invstd_e, wd, bd, relu, act_max)
            gx, gg, gb = ext().bn_act_bwd(g, x, y_d, rm, invstd_e, wd, False,
                                          relu, act_max)
        ya = ops.bn_act(xg, w, b, rm, rv, training, MOM, EPS, relu, act_max)
        ya.backward(g)
        assert torch.equal(ya, y_d), what + " autograd y"
        assert torch.equal(xg.grad, gx), what + " autograd gx"
        assert torch.equal(w.grad, gg), what + " autograd g_gamma"
        assert torch.equal(b.grad, gb), what + " autograd g_beta"


def _bn_split_check(inp, x, g, y, fwd, mean, invstd, relu, act_max, dtype,
                    what):
    """Split SyncBN form on two unequal parts of the batch."""
    n = x.shape[0]
    if n < 2:
        return
    cut = max(1, (3 * n) // 8)
    w = dev(inp.weight)
    parts = [slice(0, cut), slice(cut, n)]
    sums = [ext().bn_act_bwd_reduce(cl(g[s]), cl(x[s]), cl(y[s]), mean,
                                    invstd, relu, act_max) for s in parts]
    s_g = sums[0][0] + sums[1][0]
    s_gx = sums[0][1] + sums[1][1]
    count = float(inp.x.numel() // inp.x.shape[1])
    gxs = [ext().bn_act_bwd_apply(cl(g[s]), cl(x[s]), cl(y[s]), mean, invstd,
                                  w, s_g, s_gx, count, True, relu, act_max)
           for s in parts]
    rep, _ = eo.check_bn_bwd(torch.cat(gxs), s_gx, s_g, y, fwd, inp.g, True,
                             relu, act_max, dtype, extra=1)
    eo.assert_ok(rep, what + " split")
    # eval-mode apply ignores the sums
    gx_e = ext().bn_act_bwd_apply(cl(g[parts[1]]), cl(x[parts[1]]),
                                  cl(y[parts[1]]), mean, invstd, w, s_g, s_gx,
                                  count, False, relu, act_max)
    full_e = ext().bn_act_bwd(g, x, y, mean, invstd, w, False, relu,
                              act_max)[0]
    assert torch.equal(gx_e, full_e[parts[1]]), what + " split eval"


@pytest.mark.parametrize("C", eo.BN_CHANNELS)
@pytest.mark.parametrize("dtype", eo.BN_DTYPES, ids=name)
def test_bn_act_against_oracle(dtype, C):
    for rs in eo.BN_ROW_SHAPES:
        shape = eo.bn_shape(C, rs)
        inp = eo.bn_inputs(shape, dtype)
        x, g = cl(dev(inp.x)), cl(dev(inp.g))
        what = "bn %s %s" % (name(dtype), shape)
        mean, invstd = _bn_stats_check(inp, x, what)
        for relu, act_max in eo.BN_FLAGS:
            w2 = "%s relu=%d act_max=%g" % (what, relu, act_max)
            y, fwd = _bn_flags_check(inp, x, g, mean, invstd, relu, act_max,
                                     dtype, w2)
            _bn_split_check(inp, x, g, y, fwd, mean, invstd, relu, act_max,
                            dtype, w2)


@pytest.mark.parametrize("shape,dtype", eo.BN_BIG,
                         ids=lambda v: name(v) if isinstance(v, torch.dtype)
                         else "x".join(map(str, v)))
def test_bn_act_grid_stride(shape, dtype):
    """More rows than the capped grid covers in one pass: 18432 rows of 64
    channels for the scalar kernels (f32), 4105 rows of 520 for the vector
    kernels (bf16), the latter with a row tail."""
    inp = eo.bn_inputs(shape, dtype)
    x, g = cl(dev(inp.x)), cl(dev(inp.g))
    what = "bn big %s %s" % (name(dtype), shape)
    mean, invstd = _bn_stats_check(inp, x, what)
    for relu, act_max in eo.BN_BIG_FLAGS:
        y, fwd = _bn_flags_check(inp, x, g, mean, invstd, relu, act_max,
                                 dtype, what, autograd=False)
        _bn_split_check(inp, x, g, y, fwd, mean, invstd, relu, act_max, dtype,
                        what)


def test_bn_split_entry_points_check_their_inputs():
    """bn_act_bwd_reduce / bn_act_bwd_apply take raw pointers: a layout or
    dtype they cannot index must be refused, as bn_act_bwd refuses it."""
    inp = eo.bn_inputs((3, 8, 5, 5), torch.bfloat16)
    x, g = cl(dev(inp.x)), cl(dev(inp.g))
    mean, invstd = ext().bn_stats_finalize(
        x, torch.empty(0, device="cuda"), torch.empty(0, device="cuda"), MOM,
        EPS)
    w = dev(inp.weight)
    y = ext().bn_act_fwd(x, mean, invstd, w, dev(inp.bias), True, 2.0)
    s_g, s_gx = ext().bn_act_bwd_reduce(g, x, y, mean, invstd, True, 2.0)
    nchw = g.contiguous()
    for bad in ((nchw, x, y), (g, x.contiguous(), y), (g, x, y.contiguous()),
                (g.float(), x, y), (g, x, y[:2])):
        with pytest.raises(RuntimeError):
            ext().bn_act_bwd_reduce(*bad, mean, invstd, True, 2.0)
        with pytest.raises(RuntimeError):
            ext().bn_act_bwd_apply(*bad, mean, invstd, w, s_g, s_gx, 75.0,
                                   True, True, 2.0)
    with pytest.raises(RuntimeError):
        ext().bn_act_bwd_reduce(g, x, y, mean[:4], invstd, True, 2.0)
    with pytest.raises(RuntimeError):
        ext().bn_act_bwd_apply(g, x, y, mean, invstd, w, s_g.double(), s_gx,
                               75.0, True, True, 2.0)


# ---------------------------------------------------------------------------
# relu_clip
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", eo.BN_DTYPES, ids=name)
def test_relu_clip_against_oracle(dtype):
    x, g = eo.relu_clip_inputs(dtype)
    xd = cl(dev(x))            # channels_last y ...
    gd = dev(g).contiguous()   # ... with an NCHW g
    for relu in (True, False):
        for act_max in eo.ACT_MAXES:
            what = "relu_clip %s relu=%d act_max=%g" % (name(dtype), relu,
                                                        act_max)
            y = ext().relu_clip_fwd(xd, relu, act_max)
            assert y.is_contiguous(memory_format=torch.channels_last)
            ref = eo.relu_clip(x, relu, act_max, dtype)
            eo.assert_ok(eo.check_act_fwd(y, ref, relu, act_max, dtype), what)
            gx = ext().relu_clip_bwd(gd, y, relu, act_max)
            eo.assert_ok(eo.check_relu_clip_bwd(gx, y, ref, g, relu, act_max,
                                                dtype), what + " bwd")
            xa = xd.clone().requires_grad_(True)
            ops.relu_clip(xa, act_max, relu).backward(gd)
            assert torch.equal(xa.grad, gx), what + " autograd"


# ---------------------------------------------------------------------------
# activations and SE gating
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("act", eo.ACTS)
@pytest.mark.parametrize("dtype", eo.BN_DTYPES, ids=name)
def test_activation_against_oracle(dtype, act):
    x, g = eo.act_inputs(dtype)
    idx = ops.functional._ACT_IDS[act]
    xd = cl(dev(x))
    gd = dev(g).contiguous()   # NCHW g, channels_last x
    y = ext().act_fwd(xd, idx)
    gx = ext().act_bwd(gd, xd, idx)
    # the derivative itself (g = 1)
    d = ext().act_bwd(torch.ones_like(xd), xd, idx)
    assert gx.is_contiguous(memory_format=torch.channels_last)
    if dtype == torch.float32:
        # the figures recorded in profiles/epilogue_oracle.md
        print("measured %s: fwd %.3f ulp, bwd %.3f ulp of max(|ref|, 1)" % (
            act, float(eo.ulp_error(y, eo.act_fwd(x, act), 1.0).max()),
            float(eo.ulp_error(d, eo.act_deriv(x, act), 1.0).max())))
    eo.assert_ok(eo.check_act(y, gx, x, g, act, dtype),
                 "%s %s" % (act, name(dtype)))
    eo.assert_ok(eo.check_act(None, d, x, torch.ones_like(x), act, dtype),
                 "%s' %s" % (act, name(dtype)))
    xa = xd.clone().requires_grad_(True)
    ya = ops.functional.ActFn.apply(xa, act)
    ya.backward(gd)
    assert torch.equal(ya, y) and torch.equal(xa.grad, gx)


@pytest.mark.parametrize("gate", ["sigmoid", "hard_sigmoid"])
@pytest.mark.parametrize("dtype", eo.BN_DTYPES, ids=name)
def test_se_scale_against_oracle(dtype, gate):
    for C in (5, 64, 72):
        for hw in (1, 49):
            x, s, g = eo.se_inputs(C, hw, dtype)
            xd = cl(dev(x)).requires_grad_(True)
            sd = dev(s).requires_grad_(True)
            y = ops.se_scale(xd, sd, gate)
            y.backward(dev(g).contiguous())
            eo.assert_ok(eo.check_se(y, xd.grad, sd.grad, x, s, g, gate,
                                     dtype),
                         "se %s %s C=%d hw=%d" % (gate, name(dtype), C, hw))


# ---------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("k,s,p", eo.POOL_PARAMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=name)
def test_pools_against_oracle(dtype, k, s, p):
    for H, W in eo.POOL_HW:
        for C in eo.POOL_C:
            x, xa, g = eo.pool_inputs(C, H, W, k, s, p, dtype)
            what = "%s k%d s%d p%d %dx%d C=%d" % (name(dtype), k, s, p, H, W,
                                                  C)
            gd = cl(dev(g))
            y, code = ext().maxpool_fwd(cl(dev(x)), k, s, p)
            gx = ext().maxpool_bwd(gd, code, H, W, k, s, p)
            assert gx.shape == x.shape
            eo.assert_ok(eo.check_maxpool(y, gx, x, g, k, s, p, dtype),
                         "maxpool " + what)
            ya = ext().avgpool_fwd(cl(dev(xa)), k, s, p)
            gxa = ext().avgpool_bwd(gd, H, W, k, s, p)
            assert gxa.shape == xa.shape
            eo.assert_ok(eo.check_avgpool(ya, gxa, xa, g, k, s, p, dtype),
                         "avgpool " + what)
    # and through autograd (the atomic accumulation order is free, so the
    # bound again, not bit equality)
    xg = cl(dev(x)).requires_grad_(True)
    ops.maxpool_nhwc(xg, k, s, p).backward(dev(g).contiguous())
    eo.assert_ok(eo.check_maxpool(None, xg.grad, x, g, k, s, p, dtype),
                 "maxpool autograd " + what)
    xg = cl(dev(xa)).requires_grad_(True)
    ops.avgpool_nhwc(xg, k, s, p).backward(dev(g).contiguous())
    eo.assert_ok(eo.check_avgpool(None, xg.grad, xa, g, k, s, p, dtype),
                 "avgpool autograd " + what)


# ---------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("rows,cols", eo.XENT_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=name)
def test_softmax_xent_against_oracle(dtype, rows, cols, monkeypatch):
    logits, target = eo.xent_inputs(rows, cols, dtype)
    ld, td = dev(logits), dev(target)
    what = "xent %s %dx%d" % (name(dtype), rows, cols)
    loss, sm = ext().softmax_xent_fwd(ld, td)
    grad = ext().softmax_xent_bwd(sm, td, eo.XENT_SCALE)
    eo.assert_ok(eo.check_xent(loss, sm, grad, logits, target, eo.XENT_SCALE,
                               dtype), what)
    scale_t = torch.tensor([eo.XENT_SCALE], device="cuda", dtype=torch.float32)
    grad_t = ext().softmax_xent_bwd_t(sm, td, scale_t)
    assert torch.equal(grad, grad_t), what + ": host- and device-scalar " \
        "backward differ in %d elements" % int((grad != grad_t).sum())

    # ops.cross_entropy(...).backward() takes the device-scalar route
    mod = ext()
    calls = []
    real_t = mod.softmax_xent_bwd_t

    def host_route(*a):
        raise AssertionError("backward took the host-scalar route")

    def device_route(*a):
        calls.append(1)
        return real_t(*a)

    monkeypatch.setattr(mod, "softmax_xent_bwd", host_route)
    monkeypatch.setattr(mod, "softmax_xent_bwd_t", device_route)
    la = ld.clone().requires_grad_(True)
    la_loss = ops.cross_entropy(la, td)
    (la_loss * scale_t[0]).backward()
    assert calls == [1]
    # (the loss is an atomic sum: the bound, not the bits)
    eo.assert_ok(eo.check_xent(la_loss, None, None, logits, target,
                               eo.XENT_SCALE, dtype), what + " autograd loss")
    assert torch.equal(la.grad, grad), what + " autograd"
