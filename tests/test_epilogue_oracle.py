"""CPU tests of the epilogue oracle (tests/epilogue_oracle.py).

Three things are shown without a GPU: the oracle agrees with fp64 torch
autograd of the eager composition; the project's CPU fallback path meets the
same checks the HIP kernels have to meet; and every check can fail, by
feeding it a result that is wrong in the way a kernel could be wrong.
"""

import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import epilogue_oracle as eo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

EPS = 1e-5
MOM = 0.1
CPU_DTYPES = (torch.float32, torch.bfloat16)


def close64(a, b, tol=1e-11):
    a, b = eo.d64(a), eo.d64(b)
    return float((a - b).abs().max()) <= tol * (1 + float(b.abs().max()))


# ---------------------------------------------------------------------------
# the oracle against fp64 autograd
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(3, 10, 5, 5), (7, 65)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu,act_max", [(True, 0.7), (False, 2.0),
                                          (True, 0.0)])
def test_bn_oracle_matches_fp64_autograd(shape, training, relu, act_max):
    inp = eo.bn_inputs(shape, torch.float32)
    x = inp.x.double().requires_grad_(True)
    w = inp.weight.double().requires_grad_(True)
    b = inp.bias.double().requires_grad_(True)
    rm, rv = inp.running_mean.double(), inp.running_var.double()
    rm_t, rv_t = rm.clone(), rv.clone()
    z = F.batch_norm(x, rm_t, rv_t, w, b, training, MOM, EPS)
    y = F.relu(z) if relu else z
    if act_max > 0:
        y = y.clamp(max=act_max)
    g = inp.g.double()
    y.backward(g)

    st = eo.bn_stats(inp.x, EPS)
    if training:
        mean, invstd = st.mean, st.invstd
        new_m, new_v, _, _ = eo.running_update(st, rm, rv, MOM)
        assert close64(rm_t, new_m) and close64(rv_t, new_v)
    else:
        mean, invstd = rm, (rv + EPS).rsqrt()
    fwd = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias, relu,
                        act_max, torch.float32)
    ref = eo.bn_act_bwd(fwd, g, fwd.mask, training, torch.float32)
    assert close64(eo.rows_c(y), fwd.y)
    assert close64(eo.rows_c(x.grad), ref.gx)
    assert close64(w.grad, ref.g_gamma)
    assert close64(b.grad, ref.g_beta)


def test_split_oracle_equals_full_batch():
    """Sums over two unequal parts and count = total rows give the
    full-batch gradient."""
    inp = eo.bn_inputs((7, 10), torch.float32)
    mean, invstd = eo.f32_stats(inp.x)
    full = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias, True, 0.7,
                         torch.float32)
    ref = eo.bn_act_bwd(full, inp.g, full.mask, True, torch.float32)
    parts, gxs = [], []
    for sl in (slice(0, 3), slice(3, 7)):
        f = eo.bn_act_fwd(inp.x[sl], mean, invstd, inp.weight, inp.bias, True,
                          0.7, torch.float32)
        parts.append((f, eo.bn_act_bwd(f, inp.g[sl], f.mask, True,
                                       torch.float32)))
    s_g = parts[0][1].g_beta + parts[1][1].g_beta
    s_gx = parts[0][1].g_gamma + parts[1][1].g_gamma
    assert close64(s_g, ref.g_beta) and close64(s_gx, ref.g_gamma)
    for (f, _), sl in zip(parts, (slice(0, 3), slice(3, 7))):
        r = eo.bn_act_bwd(f, inp.g[sl], f.mask, True, torch.float32, count=7,
                          sums=(s_g, s_gx, 0 * s_g, 0 * s_gx))
        gxs.append(r.gx)
    assert close64(torch.cat(gxs), ref.gx)


@pytest.mark.parametrize("act,fn", [
    ("swish", F.silu), ("mish", F.mish), ("hardswish", F.hardswish),
    # F.hardsigmoid's fp64 backward multiplies by an f32 1/6 (2e-8 off)
    ("hardsigmoid", lambda v: F.relu6(v + 3) / 6), ("sigmoid", torch.sigmoid)])
def test_activation_oracle_matches_fp64_autograd(act, fn):
    gen = torch.Generator().manual_seed(3)
    # no point exactly on a kink: autograd's one-sided choice there is its own
    x = (torch.randn(4000, generator=gen, dtype=torch.float64) * 6)
    x = x.requires_grad_(True)
    g = torch.randn(4000, generator=gen, dtype=torch.float64)
    y = fn(x)
    y.backward(g)
    assert close64(y, eo.act_fwd(x, act))
    assert close64(x.grad, g * eo.act_deriv(x, act))


def test_activation_oracle_kinks():
    x = torch.tensor([-3.0, 3.0, 0.0])
    assert eo.act_deriv(x, "hardswish").tolist() == [0.0, 1.0, 0.5]
    assert eo.act_deriv(x, "hardsigmoid").tolist() == [0.0, 0.0, 1.0 / 6]
    assert eo.act_fwd(x, "hardswish").tolist() == [0.0, 3.0, 0.0]
    assert eo.act_fwd(x, "hardsigmoid").tolist() == [0.0, 1.0, 0.5]


def test_se_oracle_matches_fp64_autograd():
    x, s, g = eo.se_inputs(5, 49, torch.float32)
    for gate, fn in (("sigmoid", torch.sigmoid),
                     ("hardsigmoid", lambda v: F.relu6(v + 3) / 6)):
        xe = x.double().requires_grad_(True)
        se = (s.double() * 0.9).requires_grad_(True)   # off the kinks
        (xe * fn(se)).backward(g.double())
        r = eo.se_scale(x, s.double() * 0.9, g, gate, torch.float32)
        assert close64(xe.grad, r.gx) and close64(se.grad, r.gs)


@pytest.mark.parametrize("k,s,p", eo.POOL_PARAMS)
def test_pool_oracles_match_fp64_autograd(k, s, p):
    for H, W in eo.POOL_HW:
        _, xa, g = eo.pool_inputs(5, H, W, k, s, p, torch.float32)
        xe = xa.double().requires_grad_(True)
        y = F.avg_pool2d(xe, k, s, p, count_include_pad=True)
        y.backward(g.double())
        yr, gxr, _, _ = eo.avgpool(xa, g, k, s, p)
        assert close64(y, yr) and close64(xe.grad, gxr), (H, W)


@pytest.mark.parametrize("rows,cols", [(5, 10), (3, 65)])
def test_xent_oracle_matches_fp64_autograd(rows, cols):
    logits, target = eo.xent_inputs(rows, cols, torch.float32)
    le = logits.double().requires_grad_(True)
    loss = F.cross_entropy(le, target)
    (loss * eo.XENT_SCALE).backward()
    r = eo.softmax_xent(logits, target, eo.XENT_SCALE, torch.float32)
    assert close64(loss, r.loss)
    assert close64(le.grad, r.grad)
    assert close64(F.softmax(le, 1), r.p)


# ---------------------------------------------------------------------------
# the CPU fallback path through the same checks
# ---------------------------------------------------------------------------


def _cpu_bn(inp, training, relu, act_max, dtype):
    x = inp.x.clone().requires_grad_(True)
    w = inp.weight.clone().requires_grad_(True)
    b = inp.bias.clone().requires_grad_(True)
    rm, rv = inp.running_mean.clone(), inp.running_var.clone()
    y = ops.bn_act(x, w, b, rm, rv, training, MOM, EPS, relu, act_max)
    mean, invstd = y.grad_fn.saved_tensors[2:4]
    y.backward(inp.g)
    return SimpleNamespace(y=y.detach(), gx=x.grad, gg=w.grad, gb=b.grad,
                           rm=rm, rv=rv, mean=mean, invstd=invstd)


@pytest.mark.parametrize("dtype", CPU_DTYPES)
@pytest.mark.parametrize("shape", [(3, 10, 5, 5), (2, 65, 7, 7), (7, 8),
                                   (1, 10)])
def test_cpu_bn_act_meets_the_checks(dtype, shape):
    inp = eo.bn_inputs(shape, dtype)
    for training in (True, False):
        for relu, act_max in eo.BN_FLAGS:
            what = "cpu bn %s %s train=%s relu=%s act_max=%s" % (
                dtype, shape, training, relu, act_max)
            out = _cpu_bn(inp, training, relu, act_max, dtype)
            if training:
                assert_rep = eo.check_stats(out.mean, None, out.invstd, inp.x)
                assert_rep.update(eo.check_running(
                    out.rm, out.rv, inp.x, inp.running_mean, inp.running_var,
                    MOM))
                eo.assert_ok(assert_rep, what + " stats")
            fwd = eo.bn_act_fwd(inp.x, out.mean, out.invstd, inp.weight,
                                inp.bias, relu, act_max, dtype)
            eo.assert_ok(eo.check_act_fwd(out.y, fwd, relu, act_max, dtype),
                         what + " fwd")
            rep, _ = eo.check_bn_bwd(out.gx, out.gg, out.gb, out.y, fwd, inp.g,
                                     training, relu, act_max, dtype)
            eo.assert_ok(rep, what + " bwd")


@pytest.mark.parametrize("dtype", CPU_DTYPES)
def test_cpu_relu_clip_meets_the_checks(dtype):
    x, g = eo.relu_clip_inputs(dtype)
    for relu in (True, False):
        for act_max in eo.ACT_MAXES:
            xe = x.clone().requires_grad_(True)
            y = ops.relu_clip(xe, act_max, relu)
            y.backward(g)
            ref = eo.relu_clip(x, relu, act_max, dtype)
            what = "cpu relu_clip %s relu=%s act_max=%s" % (dtype, relu,
                                                            act_max)
            eo.assert_ok(eo.check_act_fwd(y, ref, relu, act_max, dtype), what)
            eo.assert_ok(eo.check_relu_clip_bwd(xe.grad, y, ref, g, relu,
                                                act_max, dtype), what)


@pytest.mark.parametrize("dtype", CPU_DTYPES)
@pytest.mark.parametrize("act", eo.ACTS)
def test_cpu_activations_meet_the_checks(dtype, act):
    x, g = eo.act_inputs(dtype)
    xe = x.clone().requires_grad_(True)
    y = ops.functional.ActFn.apply(xe, act)
    y.backward(g)
    eo.assert_ok(eo.check_act(y, xe.grad, x, g, act, dtype),
                 "cpu %s %s" % (act, dtype))


@pytest.mark.parametrize("dtype", CPU_DTYPES)
@pytest.mark.parametrize("k,s,p", eo.POOL_PARAMS)
def test_cpu_pools_meet_the_checks(dtype, k, s, p):
    for H, W in eo.POOL_HW:
        x, xa, g = eo.pool_inputs(5, H, W, k, s, p, dtype)
        xe = x.clone().requires_grad_(True)
        y = ops.maxpool_nhwc(xe, k, s, p)
        y.backward(g)
        eo.assert_ok(eo.check_maxpool(y, xe.grad, x, g, k, s, p, dtype),
                     "cpu maxpool")
        xe = xa.clone().requires_grad_(True)
        y = ops.avgpool_nhwc(xe, k, s, p)
        y.backward(g)
        eo.assert_ok(eo.check_avgpool(y, xe.grad, xa, g, k, s, p, dtype),
                     "cpu avgpool")


@pytest.mark.parametrize("dtype", CPU_DTYPES)
@pytest.mark.parametrize("rows,cols", [(5, 10), (3, 65), (515, 1000)])
def test_cpu_cross_entropy_meets_the_checks(dtype, rows, cols):
    logits, target = eo.xent_inputs(rows, cols, dtype)
    le = logits.clone().requires_grad_(True)
    loss = ops.cross_entropy(le, target)
    (loss * eo.XENT_SCALE).backward()
    eo.assert_ok(eo.check_xent(loss, None, le.grad, logits, target,
                               eo.XENT_SCALE, dtype), "cpu xent %s" % dtype)


# ---------------------------------------------------------------------------
# every check can fail
# ---------------------------------------------------------------------------


def _bn_case(dtype, act_max, relu=True, shape=(3, 10, 5, 5)):
    """A correct result in the kernels' formulation: y rounded to dtype, the
    mask derived from that y against the stored threshold."""
    inp = eo.bn_inputs(shape, dtype)
    mean, invstd = eo.f32_stats(inp.x)
    fwd = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias, relu,
                        act_max, dtype)
    y = fwd.y.to(dtype).view(-1, shape[1])
    return inp, fwd, y


def _bwd_with_mask(fwd, g, mask, training, dtype, **kw):
    r = eo.bn_act_bwd(fwd, g, mask, training, dtype, **kw)
    return r.gx.to(dtype), r.g_gamma.float(), r.g_beta.float()


def _check(fwd, inp, y, gx, gg, gb, training, act_max, dtype, relu=True, **kw):
    g = eo.rows_c(inp.g)
    rep, _ = eo.check_bn_bwd(gx, gg, gb, y, fwd, g, training, relu, act_max,
                             dtype, **kw)
    return rep


@pytest.mark.parametrize("dtype", CPU_DTYPES)
@pytest.mark.parametrize("training", [True, False])
def test_right_result_passes(dtype, training):
    inp, fwd, y = _bn_case(dtype, 0.7)
    eff = eo.effective_mask(y, fwd, True, 0.7, dtype)
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, eff, training, dtype)
    assert not eo.failures(eo.check_act_fwd(y, fwd, True, 0.7, dtype))
    assert not eo.failures(_check(fwd, inp, y, gx, gg, gb, training, 0.7,
                                  dtype))


@pytest.mark.parametrize("training", [True, False])
def test_rejects_ignored_clip_mask(training):
    dtype = torch.float32
    inp, fwd, y = _bn_case(dtype, 2.0)
    relu_only = (fwd.z > 0).double()
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, relu_only, training, dtype)
    bad = eo.failures(_check(fwd, inp, y, gx, gg, gb, training, 2.0, dtype))
    assert {"gx", "g_gamma", "g_beta"} <= set(bad), bad
    if not training:
        assert "n_gx_through_mask" in bad


@pytest.mark.parametrize("training", [True, False])
def test_rejects_f32_threshold_on_bf16_output(training):
    """The suspected kernel bug: act_max = 0.7 is stored as bf16 0.69921875,
    so `float(y) >= 0.7f` is never true and every saturated element passes
    its gradient."""
    dtype = torch.bfloat16
    assert eo.stored_threshold(0.7, dtype) == 0.69921875
    inp, fwd, y = _bn_case(dtype, 0.7)
    yf = y.float()
    wrong = ((yf > 0) & ~(yf >= torch.tensor(0.7, dtype=torch.float32))).double()
    saturated = (fwd.z >= 0.7) & ~fwd.band
    assert float(saturated.double().mean()) > 0.2
    assert bool((wrong[saturated] == 1).all())       # the clip never masks
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, wrong, training, dtype)
    rep = _check(fwd, inp, y, gx, gg, gb, training, 0.7, dtype)
    bad = eo.failures(rep)
    assert {"gx", "g_gamma", "g_beta"} <= set(bad), rep
    if not training:
        # every saturated element whose g * gamma * invstd is not 0 itself
        live = (eo.rows_c(inp.g) * fwd.w * fwd.invstd != 0) & saturated
        assert rep["n_gx_through_mask"] == int(live.sum()) > 0
    # the same rule is right where act_max is exact in the dtype
    inp, fwd, y = _bn_case(dtype, 2.0)
    yf = y.float()
    same = ((yf > 0) & ~(yf >= 2.0)).double()
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, same, training, dtype)
    assert not eo.failures(_check(fwd, inp, y, gx, gg, gb, training, 2.0,
                                  dtype))


def test_rejects_wrong_stored_threshold_in_forward():
    """A forward that stores act_max unrounded-then-truncated (anything but
    the dtype's own rounding) is caught by the value check."""
    dtype = torch.bfloat16
    inp, fwd, y = _bn_case(dtype, 0.7)
    y_bad = torch.where(y.float() == 0.69921875,
                        torch.tensor(0.6875, dtype=dtype), y)
    assert "y" in eo.failures(eo.check_act_fwd(y_bad, fwd, True, 0.7, dtype))


@pytest.mark.parametrize("training", [True, False])
def test_rejects_relu_mask_that_keeps_zero(training):
    """mask = 0 only for y < 0 instead of y <= 0: every rectified element
    (stored as 0) passes its gradient."""
    dtype = torch.float32
    inp, fwd, y = _bn_case(dtype, 0.0)
    wrong = (~(y.double() < 0)).double()
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, wrong, training, dtype)
    bad = eo.failures(_check(fwd, inp, y, gx, gg, gb, training, 0.0, dtype))
    assert {"gx", "g_gamma", "g_beta"} <= set(bad), bad


def test_rejects_sums_shifted_by_one_channel():
    dtype = torch.float32
    inp, fwd, y = _bn_case(dtype, 2.0)
    eff = eo.effective_mask(y, fwd, True, 2.0, dtype)
    gx, gg, gb = _bwd_with_mask(fwd, inp.g, eff, True, dtype)
    bad = eo.failures(_check(fwd, inp, y, None, gg.roll(1), gb.roll(1), True,
                             2.0, dtype))
    assert bad == ["g_beta", "g_gamma"]
    st = eo.bn_stats(inp.x)
    bad = eo.failures(eo.check_stats(st.mean.roll(1), st.var.roll(1),
                                     st.invstd.roll(1), inp.x))
    assert bad == ["invstd", "mean", "var"]


def test_rejects_dropped_row_tail():
    """75 rows: a kernel that loses the last rows % 4 = 3 of them."""
    dtype = torch.float32
    inp, fwd, y = _bn_case(dtype, 2.0)
    eff = eo.effective_mask(y, fwd, True, 2.0, dtype)
    g = eo.rows_c(inp.g)
    rows = g.shape[0]
    keep = rows - rows % 4
    assert keep == 72
    gm = (g * eff)[:keep]
    gb = gm.sum(0).float()
    gg = (gm * fwd.xhat[:keep]).sum(0).float()
    bad = eo.failures(_check(fwd, inp, y, None, gg, gb, True, 2.0, dtype))
    assert bad == ["g_beta", "g_gamma"]
    xr = eo.rows_c(inp.x)[:keep]
    bad = eo.failures(eo.check_stats(xr.mean(0), xr.var(0, unbiased=False),
                                     None, inp.x))
    assert bad == ["mean", "var"]


def test_rejects_local_count_in_split_form():
    dtype = torch.float32
    shape = (7, 10)
    inp, fwd, y = _bn_case(dtype, 0.7, shape=shape)
    mean, invstd = eo.f32_stats(inp.x)
    eff = eo.effective_mask(y, fwd, True, 0.7, dtype)
    full = eo.bn_act_bwd(fwd, inp.g, eff, True, dtype)
    sums = (full.g_beta, full.g_gamma, full.b_beta, full.b_gamma)
    good, wrong = [], []
    for sl in (slice(0, 3), slice(3, 7)):
        f = eo.bn_act_fwd(inp.x[sl], mean, invstd, inp.weight, inp.bias, True,
                          0.7, dtype)
        n_loc = sl.stop - sl.start
        good.append(eo.bn_act_bwd(f, inp.g[sl], eff[sl], True, dtype, count=7,
                                  sums=sums).gx)
        wrong.append(eo.bn_act_bwd(f, inp.g[sl], eff[sl], True, dtype,
                                   count=n_loc, sums=sums).gx)
    assert not eo.failures(_check(fwd, inp, y, torch.cat(good).float(), None,
                                  None, True, 0.7, dtype))
    assert eo.failures(_check(fwd, inp, y, torch.cat(wrong).float(), None,
                              None, True, 0.7, dtype)) == ["gx"]


def test_rejects_relu_clip_bugs():
    dtype = torch.bfloat16
    x, g = eo.relu_clip_inputs(dtype)
    ref = eo.relu_clip(x, True, 0.7, dtype)
    y = ref.y.to(dtype)
    eff = eo.effective_mask(y, ref, True, 0.7, dtype)
    assert not eo.failures(eo.check_relu_clip_bwd(
        (g.double() * eff).to(dtype), y, ref, g, True, 0.7, dtype))
    wrong = ((y.float() > 0) & ~(y.float() >= 0.7)).double()
    bad = eo.failures(eo.check_relu_clip_bwd(
        (g.double() * wrong).to(dtype), y, ref, g, True, 0.7, dtype))
    assert bad == ["gx", "n_gx_through_mask"]


def test_rejects_maxpool_scatter_to_wrong_cell():
    k, s, p = 3, 2, 1
    x, _, g = eo.pool_inputs(5, 7, 9, k, s, p, torch.float32)
    _, gx, _ = eo.maxpool(x, g, k, s, p)
    assert not eo.failures(eo.check_maxpool(None, gx.float(), x, g, k, s, p,
                                            torch.float32))
    moved = gx.roll(1, dims=3).float()
    assert abs(float(moved.sum() - gx.sum())) < 1e-4  # the old sum check passes
    assert eo.failures(eo.check_maxpool(None, moved, x, g, k, s, p,
                                        torch.float32)) == ["gx"]
    y = F.max_pool2d(x, k, s, p)
    y[0, 0, 0, 0] = x[0, 0].min()
    assert eo.failures(eo.check_maxpool(y, None, x, g, k, s, p,
                                        torch.float32)) == ["n_y"]


def test_rejects_avgpool_divided_by_valid_count():
    k, s, p = 3, 2, 1
    _, xa, g = eo.pool_inputs(5, 7, 9, k, s, p, torch.float32)
    xe = xa.clone().requires_grad_(True)
    y = F.avg_pool2d(xe, k, s, p, count_include_pad=False)
    y.backward(g)
    assert eo.failures(eo.check_avgpool(y.detach(), xe.grad, xa, g, k, s, p,
                                        torch.float32)) == ["gx", "y"]
    xe = xa.clone().requires_grad_(True)
    y = F.avg_pool2d(xe, k, s, p, count_include_pad=True)
    y.backward(g)
    assert not eo.failures(eo.check_avgpool(y.detach(), xe.grad, xa, g, k, s,
                                            p, torch.float32))


def test_rejects_xent_bugs():
    dtype = torch.float32
    logits, target = eo.xent_inputs(5, 10, dtype)
    r = eo.softmax_xent(logits, target, eo.XENT_SCALE, dtype)
    assert not eo.failures(eo.check_xent(r.loss.float(), r.p.float(),
                                         r.grad.float(), logits, target,
                                         eo.XENT_SCALE, dtype))
    onehot_next = F.one_hot((target + 1) % 10, 10).double()
    shifted = ((r.p - onehot_next) * eo.XENT_SCALE / 5).float()
    assert eo.failures(eo.check_xent(None, None, shifted, logits, target,
                                     eo.XENT_SCALE, dtype)) == ["grad"]
    twice = (r.grad * eo.XENT_SCALE).float()
    assert eo.failures(eo.check_xent(None, None, twice, logits, target,
                                     eo.XENT_SCALE, dtype)) == ["grad"]
    # no max subtraction: exp overflows on a row shifted by +90
    hot = logits.clone()
    hot[0] += 90 - hot[0].max()
    e = hot.exp()
    assert eo.failures(eo.check_xent(None, e / e.sum(1, keepdim=True), None,
                                     hot, target, eo.XENT_SCALE,
                                     dtype)) == ["softmax"]
    sum_not_mean = (r.loss * 5).float()
    assert eo.failures(eo.check_xent(sum_not_mean, None, None, logits, target,
                                     eo.XENT_SCALE, dtype)) == ["loss"]


def test_rejects_activation_bugs():
    dtype = torch.float32
    x, g = eo.act_inputs(dtype)
    # hardswish derivative without the kink at +3 (2x+3)/6 beyond it
    d = (2 * x.double() + 3) / 6 * (x.double() > -3)
    assert eo.failures(eo.check_act(None, (g.double() * d).float(), x, g,
                                    "hardswish", dtype)) == ["gx"]
    # mish forward mistaken for swish
    assert eo.failures(eo.check_act(eo.act_fwd(x, "swish").float(), None, x,
                                    g, "mish", dtype)) == ["y"]
    # hardsigmoid derivative 1/6 ON the kinks
    d = ((x.double() >= -3) & (x.double() <= 3)).double() / 6
    assert eo.failures(eo.check_act(None, (g.double() * d).float(), x, g,
                                    "hardsigmoid", dtype)) == ["gx"]


# ---------------------------------------------------------------------------
# the ambiguous band stays small on every input set of the GPU tests
# ---------------------------------------------------------------------------

BAND_CAP = 0.01


@pytest.mark.parametrize("dtype", eo.BN_DTYPES)
def test_ambiguous_share_of_bn_inputs(dtype):
    worst = 0.0
    for C in eo.BN_CHANNELS:
        for rs in eo.BN_ROW_SHAPES:
            shape = eo.bn_shape(C, rs)
            inp = eo.bn_inputs(shape, dtype)
            mean, invstd = eo.f32_stats(inp.x)
            for relu, act_max in eo.BN_FLAGS:
                fwd = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias,
                                    relu, act_max, dtype)
                share = eo.band_share(fwd.band)
                worst = max(worst, share)
                assert share <= BAND_CAP, (shape, relu, act_max, share)
    print("worst ambiguous share, bn %s: %.4f" % (dtype, worst))


def test_ambiguous_share_of_big_bn_inputs():
    for shape, dtype in eo.BN_BIG:
        inp = eo.bn_inputs(shape, dtype)
        mean, invstd = eo.f32_stats(inp.x)
        for relu, act_max in eo.BN_BIG_FLAGS:
            fwd = eo.bn_act_fwd(inp.x, mean, invstd, inp.weight, inp.bias,
                                relu, act_max, dtype)
            share = eo.band_share(fwd.band)
            print("ambiguous share %s %s: %.5f" % (shape, dtype, share))
            assert share <= BAND_CAP, (shape, dtype, share)


@pytest.mark.parametrize("dtype", eo.BN_DTYPES)
def test_ambiguous_share_of_relu_clip_inputs(dtype):
    x, _ = eo.relu_clip_inputs(dtype)
    for relu in (True, False):
        for act_max in eo.ACT_MAXES:
            share = eo.band_share(eo.relu_clip(x, relu, act_max, dtype).band)
            print("ambiguous share relu_clip %s %s: %.5f" % (dtype, act_max,
                                                             share))
            assert share <= BAND_CAP, (dtype, relu, act_max, share)
