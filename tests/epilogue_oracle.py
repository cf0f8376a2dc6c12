"""fp64 oracle for the epilogue kernels: BatchNorm + ReLU + clip, relu_clip,
the EfficientNet activations, SE gating, the generic pools and softmax
cross-entropy.

A plain helper module (CPU tensors only, everything in fp64) shared by
test_epilogue_oracle.py, which proves on the CPU that each check below can
fail, and by test_epilogue_gpu.py. It never calls noisynet_amd.ops: it is the
independent side of every comparison.

Bounds. Every comparison is

    |got - ref| <= U_OUT[dtype] * |ref| + gamma(n) * A

U_OUT is one rounding to the output dtype, n the number of f32 roundings
behind the value (the length of an accumulation, in any order, plus the
chained elementwise operations in front of it) and A the fp64 sum of the
absolute values of the terms. Where a result is computed from other rounded
results (the train-mode gx from the per-channel sums, the loss gradient from
the stored softmax) the bounds of those are propagated through the formula.

Masks. The activation mask is defined on the fp64 PRE-activation z (0 < z if
relu, z < act_max if clipped), never on a rounded output. Kernels re-derive
it from the stored y, so where z is within rounding of a threshold the two
may differ legitimately: that set is the ambiguous band, inside it the mask
implied by the kernel's own y is accepted, outside it the oracle's binds.
"""

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from fused_noise_oracle import U_OUT, gamma

ACTS = ("swish", "mish", "hardswish", "hardsigmoid", "sigmoid")

U32 = U_OUT[torch.float32]

# Absolute floor of one output rounding. U_OUT * |ref| holds for normal
# results only: an fp16 result below 2^-14 is rounded on the subnormal grid
# (half a step = 2^-25), and an f32 or bf16 result below the smallest normal
# 2^-126 may be flushed to zero by the f32 arithmetic in front of it.
OUT_FLOOR = {
    torch.float16: 2.0 ** -25,
    torch.bfloat16: 2.0 ** -126,
    torch.float32: 2.0 ** -126,
}


def out_round(ref, dtype):
    """One rounding of ``ref`` to ``dtype``."""
    return U_OUT[dtype] * ref.abs() + OUT_FLOOR[dtype]


# ---------------------------------------------------------------------------
# layout helpers
# ---------------------------------------------------------------------------


def rows_c(t):
    """[N,C,H,W] (any memory format) or [N,C] -> fp64 [rows, C] on the CPU,
    row = (n, h, w) in row-major order (the kernels' NHWC index space)."""
    t = t.detach().cpu().double()
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.contiguous()


def d64(t):
    return t.detach().cpu().double()


def stored_threshold(act_max, dtype):
    """act_max as the forward stores it: f32, then one rounding to dtype."""
    return float(torch.tensor(float(act_max), dtype=torch.float32).to(dtype))


def ulp_below(v, dtype):
    """Spacing of ``dtype`` just below |v| (v > 0)."""
    t = torch.tensor(float(v), dtype=torch.float32).to(dtype)
    lo = torch.nextafter(t, torch.zeros_like(t))
    return float(t.double() - lo.double())


# ---------------------------------------------------------------------------
# generic comparison
# ---------------------------------------------------------------------------


def ratio(got, ref, bound):
    """max |got-ref| / bound; 0/0 counts as 0, a non-finite value as inf."""
    got, ref = d64(got), d64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err),
                    err / bound.clamp_min(1e-300))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def within(got, ref, bound, what):
    r = ratio(got, ref, bound)
    print("%s: worst |err|/bound = %.3g" % (what, r))
    assert r <= 1.0, "%s: |err| reaches %.3g x the derived bound" % (what, r)
    return r


def elementwise_bound(ref, A, dtype, n=1):
    """n chained f32 operations on terms of magnitude A, one output rounding."""
    return out_round(ref, dtype) + gamma(n) * A


# ---------------------------------------------------------------------------
# BatchNorm statistics
# ---------------------------------------------------------------------------


def bn_stats(x, eps=1e-5):
    """fp64 per-channel mean, biased var and invstd over the rows of x, with
    the bounds of an f32 kernel that forms them as sum/n and sumsq/n - mean^2
    (any summation order)."""
    x = rows_c(x)
    n = x.shape[0]
    mean = x.mean(0)
    ex2 = (x * x).mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = (var + eps).rsqrt()
    b_mean = U32 * mean.abs() + gamma(n) * x.abs().mean(0)
    # sumsq: n products and n adds; then /n, mean*mean, the subtraction
    b_var = (gamma(n + 4) * (ex2 + mean * mean)
             + 2 * mean.abs() * b_mean + b_mean ** 2)
    # d rsqrt(v+eps) = -0.5 (v+eps)^-1.5 dv, plus the rsqrt itself (2 ulp)
    # and second order in dv (the bound is only useful while dv << v+eps)
    rel = b_var / (var + eps)
    b_invstd = invstd * (0.5 * rel + rel * rel) + gamma(2) * invstd
    return SimpleNamespace(mean=mean, var=var, invstd=invstd, ex2=ex2, n=n,
                           b_mean=b_mean, b_var=b_var, b_invstd=b_invstd)


def running_update(st, running_mean, running_var, momentum):
    """Running buffers after one training step: (1-m)*old + m*new with the
    unbiased variance n/(n-1) (n/1 for a single row, as the project does).
    Returns (mean, var, bound_mean, bound_var)."""
    rm, rv = d64(running_mean), d64(running_var)
    unbias = st.n / max(st.n - 1.0, 1.0)
    new_m = rm * (1 - momentum) + momentum * st.mean
    new_v = rv * (1 - momentum) + momentum * st.var * unbias
    # momentum to f32, 1-momentum, two products, one add (+ unbias product)
    b_m = momentum * st.b_mean + gamma(6) * (
        rm.abs() * (1 - momentum) + momentum * st.mean.abs())
    b_v = momentum * unbias * st.b_var + gamma(7) * (
        rv.abs() * (1 - momentum) + momentum * st.var * unbias)
    return new_m, new_v, b_m, b_v


# ---------------------------------------------------------------------------
# BN + ReLU + clip
# ---------------------------------------------------------------------------


def act_masks(z, A, relu, act_max, dtype):
    """(mask, band) for pre-activation z with sum of absolute terms A (see
    bn_act_fwd). mask is fp64 0/1.

    band: z within gamma(1)*A of 0 or of act_max (sub, two products and an
    add in f32 are four roundings of 2^-24 each: the kernel's own z may fall
    on the other side), 0 < z below the smallest normal of the dtype (may
    round to 0), or z within one ulp of the storage dtype below act_max
    (rounds up onto the stored threshold, or the threshold itself rounded
    down into that interval)."""
    slack = gamma(1) * A
    mask = torch.ones_like(z)
    band = torch.zeros_like(z, dtype=torch.bool)
    if relu:
        mask = mask * (z > 0).double()
        band |= z.abs() <= slack
        band |= (z > 0) & (z < torch.finfo(dtype).tiny)
    if act_max > 0:
        mask = mask * (z < act_max).double()
        band |= (z - act_max).abs() <= slack
        thr = min(stored_threshold(act_max, dtype), float(act_max))
        band |= (z >= thr - ulp_below(thr, dtype)) & (z < act_max)
    return mask, band


def mask_from_y(y, relu, act_max, dtype):
    """The mask a kernel derives from its stored output: 0 < y, and y below
    the threshold AS STORED (act_max rounded the way the forward rounded
    it). Elementwise, in y's own layout."""
    y = d64(y)
    m = torch.ones_like(y)
    if relu:
        m = m * (y > 0).double()
    if act_max > 0:
        m = m * (y < stored_threshold(act_max, dtype)).double()
    return m


def resolve_mask(mask, band, y_mask):
    """Oracle mask outside the band, the kernel's own inside."""
    return torch.where(band, y_mask, mask)


def bn_act_fwd(x, mean, invstd, weight, bias, relu, act_max, dtype):
    """BN + act forward as [rows, C] from GIVEN mean/invstd (fp64 of whatever
    the kernel under test is fed). Returns z, y, A (sum of absolute terms of
    z), the mask on z, the ambiguous band and the bound of y."""
    x = rows_c(x)
    mean, invstd, w, b = d64(mean), d64(invstd), d64(weight), d64(bias)
    xhat = (x - mean) * invstd
    z = xhat * w + b
    A = (x.abs() + mean.abs()) * invstd * w.abs() + b.abs()
    y = z.clamp_min(0) if relu else z.clone()
    if act_max > 0:
        y = y.clamp_max(act_max)
    mask, band = act_masks(z, A, relu, act_max, dtype)
    # sub, two products, add: four roundings of 2^-24 = gamma(1). A
    # saturated output is the stored threshold itself (one rounding of
    # act_max, covered by U_OUT).
    bound = out_round(y, dtype) + gamma(1) * A
    return SimpleNamespace(x=x, xhat=xhat, z=z, y=y, A=A, mask=mask,
                           band=band, bound=bound, mean=mean, invstd=invstd,
                           w=w)


def bn_act_bwd(fwd, g, mask, training, dtype, count=None, sums=None,
               extra=0):
    """BN + act backward from a bn_act_fwd result and a 0/1 mask.

    g_beta = sum g*mask, g_gamma = sum g*mask*xhat (over this tensor's rows);
    train: gx = gamma*invstd*(g*mask - S_g/count - xhat*S_gx/count)
    eval:  gx = gamma*invstd*g*mask
    ``count``/``sums`` give the split SyncBN form: S_g, S_gx summed over all
    parts (``sums`` = (S_g, S_gx, bound_S_g, bound_S_gx)) and count = total
    rows. By default they are this tensor's own. ``extra`` counts further
    f32 adds behind the sums under test (partials added by the caller).
    Returns gx, g_gamma, g_beta and their bounds."""
    g = rows_c(g)
    rows = g.shape[0]
    gm = g * mask
    g_beta = gm.sum(0)
    g_gamma = (gm * fwd.xhat).sum(0)
    # any-order f32 sum of `rows` terms; each g_gamma term carries the sub
    # and two products of xhat
    b_beta = U32 * g_beta.abs() + gamma(rows + extra) * gm.abs().sum(0)
    xh_abs = (fwd.x.abs() + fwd.mean.abs()) * fwd.invstd
    b_gamma = U32 * g_gamma.abs() + gamma(rows + 3 + extra) * (
        gm.abs() * xh_abs).sum(0)
    gi = fwd.w * fwd.invstd
    if not training:
        gx = gm * gi
        b_gx = elementwise_bound(gx, gx.abs(), dtype)
    else:
        if sums is None:
            s_g, s_gx, b_sg, b_sgx = g_beta, g_gamma, b_beta, b_gamma
            count = rows
        else:
            s_g, s_gx, b_sg, b_sgx = sums
        gx = gi * (gm - s_g / count - fwd.xhat * s_gx / count)
        # 1/count, gamma*invstd, xhat (3), four products, two subtractions
        a_el = gi.abs() * (gm.abs() + s_g.abs() / count
                           + xh_abs * s_gx.abs() / count)
        b_gx = (out_round(gx, dtype) + gamma(10) * a_el
                + gi.abs() * (b_sg + xh_abs * b_sgx) / count)
    return SimpleNamespace(gx=gx, g_gamma=g_gamma, g_beta=g_beta, b_gx=b_gx,
                           b_gamma=b_gamma, b_beta=b_beta)


def band_share(band):
    return float(band.double().mean()) if band.numel() else 0.0


# ---------------------------------------------------------------------------
# relu_clip
# ---------------------------------------------------------------------------


def relu_clip(x, relu, act_max, dtype):
    """Flat fp64 forward of relu+clip on an already-rounded x (exact up to
    the stored threshold), with mask and band."""
    z = d64(x)
    y = z.clamp_min(0) if relu else z.clone()
    if act_max > 0:
        y = y.clamp_max(act_max)
    # x is exact in the dtype: no evaluation error, only the storage band
    mask, band = act_masks(z, torch.zeros_like(z), relu, act_max, dtype)
    return SimpleNamespace(z=z, y=y, mask=mask, band=band,
                           bound=out_round(y, dtype))


def relu_clip_bwd(g, mask, dtype):
    gx = d64(g) * mask
    return gx, torch.zeros_like(gx)  # g*1 or g*0: exact


# ---------------------------------------------------------------------------
# activations (closed form) and SE gating
# ---------------------------------------------------------------------------


def act_fwd(x, act):
    x = d64(x)
    if act == "swish":
        return x * torch.sigmoid(x)
    if act == "mish":
        return x * torch.tanh(F.softplus(x, threshold=1e9))
    if act == "hardswish":
        return x * (x + 3).clamp(0, 6) / 6
    if act == "hardsigmoid":
        return (x + 3).clamp(0, 6) / 6
    assert act == "sigmoid", act
    return torch.sigmoid(x)


def act_deriv(x, act):
    """d act/dx in closed form. At the kinks the one-sided value the project
    defines: hardswish' = 0 for x <= -3, 1 for x >= 3; hardsigmoid' = 1/6 on
    the open interval (-3, 3) only."""
    x = d64(x)
    s = torch.sigmoid(x)
    if act == "swish":
        return s * (1 + x * (1 - s))
    if act == "mish":
        t = torch.tanh(F.softplus(x, threshold=1e9))
        return t + x * s * (1 - t * t)
    if act == "hardswish":
        return torch.where(x <= -3, torch.zeros_like(x),
                           torch.where(x >= 3, torch.ones_like(x),
                                       (2 * x + 3) / 6))
    if act == "hardsigmoid":
        return ((x > -3) & (x < 3)).double() / 6
    assert act == "sigmoid", act
    return s * (1 - s)


def act_terms(x, act):
    """Sum of absolute terms of (forward, derivative) for the piecewise
    activations (exact arithmetic apart from f32 rounding)."""
    x = d64(x).abs()
    if act == "hardswish":
        return x * (x + 3).clamp_max(6) / 6, (2 * x + 3) / 6
    assert act == "hardsigmoid", act
    return (x + 3).clamp_max(6) / 6, torch.full_like(x, 1.0 / 6)


def piecewise_bounds(x, g, act, dtype):
    """Bounds of y and gx for hardswish/hardsigmoid: add, clamp, products
    (<= 4 roundings of 2^-24 = gamma(1)), one output rounding."""
    a_f, a_d = act_terms(x, act)
    y, d = act_fwd(x, act), act_deriv(x, act)
    gx = d64(g) * d
    return (elementwise_bound(y, a_f, dtype),
            elementwise_bound(gx, d64(g).abs() * a_d, dtype))


def ulp_error(got, ref, floor):
    """|got-ref| in f32 ulps of max(|ref|, floor) (ulp of v: 2^(floor(log2
    v) - 23))."""
    got, ref = d64(got), d64(ref)
    mag = ref.abs().clamp_min(floor)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 23)
    return (got - ref).abs() / ulp


def se_scale(x, s, g, gate, dtype):
    """SE gating y = x*gate(s[b,c]), gx = g*gate, gs = (sum_hw g*x)*gate'(s),
    x/g as [B,C,H,W], s as [B,C,1,1]. Returns values and the sums of absolute
    terms; gate error is the caller's (measured for sigmoid, derived for
    hardsigmoid)."""
    x, s, g = d64(x), d64(s).reshape(x.shape[0], x.shape[1], 1, 1), d64(g)
    gate, dgate = act_fwd(s, gate), act_deriv(s, gate)
    hw = x.shape[2] * x.shape[3]
    dot = (g * x).sum((2, 3), keepdim=True)
    dot_abs = (g * x).abs().sum((2, 3), keepdim=True)
    return SimpleNamespace(y=x * gate, gx=g * gate, gs=dot * dgate,
                           gate=gate, dgate=dgate, dot_abs=dot_abs, hw=hw)


# ---------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------


def maxpool(x, g, k, stride, pad):
    """fp64 F.max_pool2d, its autograd gradient and the same scatter of |g|
    (the sum of absolute terms of the gradient), NCHW."""
    x = d64(x).contiguous().requires_grad_(True)
    y = F.max_pool2d(x, k, stride, pad)
    (gx,) = torch.autograd.grad(y, x, d64(g).contiguous(), retain_graph=True)
    (gabs,) = torch.autograd.grad(y, x, d64(g).abs().contiguous())
    return y.detach(), gx, gabs


def avgpool(x, g, k, stride, pad):
    """fp64 avg pool with count_include_pad=True, written out: every window
    divides by k*k. Returns y, gx and the sums of absolute terms of both."""
    x, g = d64(x), d64(g)
    ones = torch.ones(x.shape[1], 1, k, k, dtype=torch.float64) / (k * k)

    def fwd(t):
        return F.conv2d(t, ones, None, stride, pad, 1, x.shape[1])

    def bwd(t):
        # every window spread over the PADDED input, then the padding cut
        # off (cells right of / below the last window stay 0)
        full = F.conv_transpose2d(t, ones, None, stride, 0, 0, x.shape[1])
        H, W = x.shape[2] + 2 * pad, x.shape[3] + 2 * pad
        full = F.pad(full, (0, max(W - full.shape[3], 0),
                            0, max(H - full.shape[2], 0)))
        return full[:, :, pad:pad + x.shape[2], pad:pad + x.shape[3]]

    return fwd(x), bwd(g), fwd(x.abs()), bwd(g.abs())


def pool_bound(ref, A, k, dtype):
    """k*k f32 adds (any order) plus the 1/(k*k) product, one rounding."""
    return out_round(ref, dtype) + gamma(k * k + 2) * A


# ---------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------


def softmax_xent(logits, target, scale, dtype):
    """Mean cross-entropy, softmax and gradient scale*(softmax-onehot)/rows.

    The kernel forms e_c = exp(l_c - max) with the fast exponential: exp2 of
    (d * log2 e), so the product's rounding (and that of the f32 log2 e)
    shifts the exponent by up to 1.5*2^-24*|d|*log2(e), a relative error of
    1.5*2^-24*|d| in e_c, plus 2 ulp for the exp2 itself:

        E(d) = (4 + 1.5*|d|) * 2^-24

    softmax = e_c/sum: E(d_c) + sum_j p_j E(d_j) + gamma(cols) for the sum
    + 2 roundings (reciprocal, product).
    loss row = -(l_t - max - log(sum)): two subtractions and a log of 2 ulp
    on terms |l_t - max| + |log sum|, plus the relative error of the sum;
    then an any-order f32 sum over rows and one division.
    The gradient is computed from the STORED softmax, so its bound carries
    that rounding: U_OUT*p*scale/rows."""
    l = d64(logits)
    rows, cols = l.shape
    t = target.detach().cpu().long()
    mx = l.max(1, keepdim=True).values
    d = l - mx
    e = d.exp()
    s = e.sum(1, keepdim=True)
    p = e / s
    E = (4 + 1.5 * d.abs()) * 2.0 ** -24
    rel_sum = (p * E).sum(1, keepdim=True) + gamma(cols)
    b_p = out_round(p, dtype) + p * (E + rel_sum + gamma(2))
    dt = d.gather(1, t[:, None])
    loss_rows = -(dt - s.log())
    b_rows = gamma(4) * (dt.abs() + s.log().abs()) + rel_sum
    loss = loss_rows.mean()
    b_loss = (U32 * loss.abs() + gamma(rows + 1) * loss_rows.abs().mean()
              + b_rows.mean())
    onehot = F.one_hot(t, cols).double()
    k = scale / rows
    grad = (p - onehot) * k
    # p as stored (b_p includes its rounding); the subtraction, scale and
    # 1/rows to f32, their product and the final product: 5 roundings of
    # 2^-24 < gamma(2); one output rounding
    b_grad = (out_round(grad, dtype) + abs(k) * b_p
              + gamma(2) * (p + onehot) * abs(k))
    return SimpleNamespace(loss=loss, b_loss=b_loss, p=p, b_p=b_p, grad=grad,
                           b_grad=b_grad)


# ---------------------------------------------------------------------------
# input sets (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------

BN_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
BN_CHANNELS = (1, 8, 10, 65, 120, 390, 520)
# 4-D rows 75 and 98, 2-D rows 1, 7 and 64: no multiple of 4 among the odd
# ones, one row, fewer rows than row groups
BN_ROW_SHAPES = ((3, 5, 5), (2, 7, 7), (1,), (7,), (64,))
BN_FLAGS = tuple((relu, am) for relu in (True, False)
                 for am in (0.0, 2.0, 0.7, 4.7))
# beyond the capped grid: the scalar kernels stride at more than 16384 rows
# of 64 channels, the vector kernels at more than 4096 rows of 520
BN_BIG = (((32, 64, 24, 24), torch.float32), ((32, 64, 24, 24), torch.bfloat16),
          ((32, 64, 24, 24), torch.float16), ((4105, 520), torch.bfloat16))
BN_BIG_FLAGS = ((True, 0.7),)


def bn_shape(C, rs):
    return (rs[0], C) + tuple(rs[1:])


# the formula's seed puts 1 of this case's 98 elements into the ambiguous
# band at act_max 0.7 (1.02 %, over the 1 % cap): another seed
BN_SEED_OVERRIDE = {(torch.bfloat16, (2, 1, 7, 7)): 5}


def bn_seed(shape, dtype):
    if (dtype, tuple(shape)) in BN_SEED_OVERRIDE:
        return BN_SEED_OVERRIDE[(dtype, tuple(shape))]
    return 1000 * BN_DTYPES.index(dtype) + 7 * shape[1] + sum(shape) % 997


def bn_inputs(shape, dtype, seed=None):
    """x with per-channel means in [-3, 3] and spreads in [0.5, 2], g ~ N(0,1),
    both rounded to dtype; f32 gamma ~ N(1, 0.5) with gamma[0] negative and
    (C >= 3) gamma[C//2] zero, beta ~ N(0.3, 0.5), running buffers."""
    gen = torch.Generator().manual_seed(
        bn_seed(shape, dtype) if seed is None else seed)
    C = shape[1]
    cshape = (1, C) + (1,) * (len(shape) - 2)
    shift = (torch.rand(C, generator=gen) * 6 - 3).view(cshape)
    spread = (torch.rand(C, generator=gen) * 1.5 + 0.5).view(cshape)
    x = torch.randn(shape, generator=gen) * spread + shift
    g = torch.randn(shape, generator=gen)
    weight = torch.randn(C, generator=gen) * 0.5 + 1.0
    weight[0] = -weight[0].abs() - 0.25
    if C >= 3:
        weight[C // 2] = 0.0
    bias = torch.randn(C, generator=gen) * 0.5 + 0.3
    return SimpleNamespace(
        x=x.to(dtype), g=g.to(dtype), weight=weight, bias=bias,
        running_mean=torch.randn(C, generator=gen),
        running_var=torch.rand(C, generator=gen) + 0.5)


def f32_stats(x, eps=1e-5):
    """The oracle's mean/invstd rounded to f32: what a correct stats kernel
    hands to the forward."""
    st = bn_stats(x, eps)
    return st.mean.float(), st.invstd.float()


RC_SHAPE = (4, 16, 9, 7)
ACT_MAXES = (0.0, 2.0, 0.7, 4.7)


def relu_clip_inputs(dtype, seed=11):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(RC_SHAPE, generator=gen) * 2.5).to(dtype)
    g = torch.randn(RC_SHAPE, generator=gen).to(dtype)
    return x, g


ACT_SHAPE = (2, 8, 16, 16)


def act_inputs(dtype, seed=12):
    """x: a grid over [-20, 20] plus exactly 0, +-3 and +-3 +- one ulp of the
    dtype, in shuffled order as a 4-D tensor; g ~ N(0,1). Both rounded."""
    gen = torch.Generator().manual_seed(seed)
    n = 1
    for s in ACT_SHAPE:
        n *= s
    three = torch.tensor(3.0, dtype=dtype)
    up = torch.nextafter(three, three * 2).float()
    dn = torch.nextafter(three, three * 0).float()
    special = torch.stack([torch.tensor(0.0), three.float(), -three.float(),
                           up, dn, -up, -dn])
    grid = torch.linspace(-20, 20, n - special.numel())
    x = torch.cat([grid, special])[torch.randperm(n, generator=gen)]
    x = x.view(ACT_SHAPE).to(dtype)
    g = torch.randn(ACT_SHAPE, generator=gen).to(dtype)
    return x, g


def se_inputs(C, hw, dtype, seed=13):
    gen = torch.Generator().manual_seed(seed + C + hw)
    h = 7 if hw == 49 else 1
    x = torch.randn(3, C, h, hw // h, generator=gen).to(dtype)
    s = (torch.randn(3, C, 1, 1, generator=gen) * 3).to(dtype)
    s.view(-1)[0] = 3.0   # the hard gate's kinks
    s.view(-1)[1] = -3.0
    g = torch.randn(3, C, h, hw // h, generator=gen).to(dtype)
    return x, s, g


POOL_PARAMS = ((3, 2, 1), (3, 1, 1), (2, 2, 0), (7, 1, 0))
POOL_HW = ((7, 9), (8, 8), (7, 7))
POOL_C = (5, 64)
POOL_N = 3


def pool_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def pool_inputs(C, H, W, k, s, p, dtype, seed=14):
    """x for the max pool: every (n, c) plane a random permutation of the
    distinct values (i - H*W/2)/8, exact in bf16, so no window has a tie.
    xa ~ N(0,1) rounded for the avg pool; g ~ N(0,1) rounded."""
    gen = torch.Generator().manual_seed(seed + C + 10 * H + W + 100 * k + s)
    hw = H * W
    perm = torch.rand(POOL_N, C, hw, generator=gen).argsort(-1)
    x = ((perm.float() - hw // 2) / 8).view(POOL_N, C, H, W).to(dtype)
    xa = torch.randn(POOL_N, C, H, W, generator=gen).to(dtype)
    g = torch.randn(POOL_N, C, pool_out(H, k, s, p), pool_out(W, k, s, p),
                    generator=gen).to(dtype)
    return x, xa, g


XENT_COLS = (10, 64, 65, 1000)
XENT_ROWS = (1, 3, 5, 515)
XENT_SHAPES = tuple((r, c) for c in XENT_COLS for r in XENT_ROWS) \
    + ((8200, 10),)
XENT_SCALE = 0.37


def xent_inputs(rows, cols, dtype, seed=15):
    """logits ~ 3*N(0,1) plus a per-row constant in [-80, 80], rounded;
    targets random with column 0 and the last column present (one row: the
    last column when cols is even, else column 0)."""
    gen = torch.Generator().manual_seed(seed + rows + 31 * cols)
    shift = torch.rand(rows, 1, generator=gen) * 160 - 80
    logits = (torch.randn(rows, cols, generator=gen) * 3 + shift).to(dtype)
    target = torch.randint(0, cols, (rows,), generator=gen)
    target[-1] = cols - 1 if (cols % 2 == 0 or rows > 1) else 0
    if rows > 1:
        target[0] = 0
    return logits, target


# ---------------------------------------------------------------------------
# checks: every function returns a report {name: value}. A name that starts
# with "n_" is a count that must be 0, every other value is |err|/bound and
# must be <= 1. failures() lists what is not met; the CPU tests feed these
# functions deliberately wrong results to show that each of them can fail.
# ---------------------------------------------------------------------------


def failures(report):
    return sorted(k for k, v in report.items()
                  if (v != 0 if k.startswith("n_") else not v <= 1.0))


def assert_ok(report, what):
    print("%s: %s" % (what, ", ".join(
        "%s %.3g" % kv for kv in sorted(report.items()))))
    bad = failures(report)
    assert not bad, "%s: %s" % (what, {k: report[k] for k in bad})


def check_stats(mean, var, invstd, x, eps=1e-5):
    """Any of mean / biased var / invstd (None to skip) against bn_stats."""
    st = bn_stats(x, eps)
    rep = {}
    if mean is not None:
        rep["mean"] = ratio(mean, st.mean, st.b_mean)
    if var is not None:
        rep["var"] = ratio(var, st.var, st.b_var)
    if invstd is not None:
        rep["invstd"] = ratio(invstd, st.invstd, st.b_invstd)
    return rep


def check_running(rm_new, rv_new, x, rm_old, rv_old, momentum, eps=1e-5):
    new_m, new_v, b_m, b_v = running_update(bn_stats(x, eps), rm_old, rv_old,
                                            momentum)
    return {"running_mean": ratio(rm_new, new_m, b_m),
            "running_var": ratio(rv_new, new_v, b_v)}


def check_act_fwd(y_got, ref, relu, act_max, dtype):
    """Output of BN+act (ref from bn_act_fwd; y_got [N,C,..]) or of relu_clip
    (ref from relu_clip; y_got any shape): value within bound, and outside
    the band the mask implied by y equals the oracle's."""
    y = rows_c(y_got) if hasattr(ref, "xhat") else d64(y_got)
    ym = mask_from_y(y, relu, act_max, dtype)
    return {"y": ratio(y, ref.y, ref.bound),
            "n_mask": int(((ym != ref.mask) & ~ref.band).sum())}


def effective_mask(y_got, ref, relu, act_max, dtype):
    y = rows_c(y_got) if hasattr(ref, "xhat") else d64(y_got)
    return resolve_mask(ref.mask, ref.band,
                        mask_from_y(y, relu, act_max, dtype))


def leaked(gx, off):
    """Number of elements the oracle masks (outside the band) whose gx is
    not exactly 0."""
    n = int((gx[off] != 0).sum())
    if n:
        print("gx != 0 on %d of the %d masked elements (%.1f %% of all %d)"
              % (n, int(off.sum()), 100.0 * n / off.numel(), off.numel()))
    return n


def check_bn_bwd(gx, g_gamma, g_beta, y_got, fwd, g, training, relu, act_max,
                 dtype, count=None, sums=None, extra=0):
    """Backward outputs (None to skip) against bn_act_bwd with the effective
    mask. In eval mode every saturated or rectified element outside the band
    must have gx exactly 0."""
    eff = effective_mask(y_got, fwd, relu, act_max, dtype)
    ref = bn_act_bwd(fwd, g, eff, training, dtype, count, sums, extra)
    rep = {}
    if gx is not None:
        rep["gx"] = ratio(rows_c(gx), ref.gx, ref.b_gx)
        if not training:
            off = (fwd.mask == 0) & ~fwd.band
            rep["n_gx_through_mask"] = leaked(rows_c(gx), off)
    if g_gamma is not None:
        rep["g_gamma"] = ratio(g_gamma, ref.g_gamma, ref.b_gamma)
    if g_beta is not None:
        rep["g_beta"] = ratio(g_beta, ref.g_beta, ref.b_beta)
    return rep, ref


def check_relu_clip_bwd(gx, y_got, ref, g, relu, act_max, dtype):
    eff = effective_mask(y_got, ref, relu, act_max, dtype)
    want, bound = relu_clip_bwd(g, eff, dtype)
    off = (ref.mask == 0) & ~ref.band
    return {"gx": ratio(gx, want, bound),
            "n_gx_through_mask": leaked(d64(gx), off)}


# Largest error of the f32 kernels' transcendental activations on the MI355X
# against this oracle, in f32 ulps of max(|ref|, 1), measured on act_inputs
# (fast exponential, logf, tanhf: no error per argument is specified). The
# floor is 1 because mish forms log(1 + e^x): for x << 0 the f32 sum 1 + e^x
# carries an absolute error of 2^-24, which is far more than one ulp of the
# tiny result, so only an absolute measure describes it. "bwd" is the
# derivative itself (g = 1). Recorded in profiles/epilogue_oracle.md.
ACT_ULPS = {
    ("swish", "fwd"): 1.421, ("swish", "bwd"): 8.171,
    ("mish", "fwd"): 8.305, ("mish", "bwd"): 4.674,
    ("sigmoid", "fwd"): 0.735, ("sigmoid", "bwd"): 0.711,
}
ACT_ABS_CAP = 1e-5  # what the older allclose(atol=1e-5) test grants


def act_tol32(ref, act, kind, A=None):
    """Absolute tolerance of the f32 evaluation of an activation (kind
    "fwd") or its derivative ("bwd"): 4x the measured error, at most 1e-5,
    for the transcendental ones; gamma(1)*A for the piecewise ones."""
    if act in ("hardswish", "hardsigmoid"):
        return gamma(1) * A
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1.0))) - 23)
    return (4.0 * ACT_ULPS[(act, kind)] * ulp).clamp_max(ACT_ABS_CAP)


def check_act(y, gx, x, g, act, dtype):
    """Activation forward and backward (gx = g * act'(x)). f32 transcendental:
    the measured bound alone; 16-bit: one rounding on top of it; piecewise:
    the derived bound."""
    yr, dr = act_fwd(x, act), act_deriv(x, act)
    gd = d64(g)
    if act in ("hardswish", "hardsigmoid"):
        b_y, b_gx = piecewise_bounds(x, g, act, dtype)
    else:
        b_y = act_tol32(yr, act, "fwd")
        if dtype != torch.float32:
            b_y = b_y + out_round(yr, dtype)
        # the product g*d is one more rounding
        b_gx = gd.abs() * act_tol32(dr, act, "bwd") + out_round(gd * dr, dtype)
    rep = {}
    if y is not None:
        rep["y"] = ratio(y, yr, b_y)
    if gx is not None:
        rep["gx"] = ratio(gx, gd * dr, b_gx)
    return rep


def check_se(y, gx, gs, x, s, g, gate, dtype):
    act = {"sigmoid": "sigmoid", "hard_sigmoid": "hardsigmoid"}[gate]
    r = se_scale(x, s, g, act, dtype)
    xd, gd = d64(x), d64(g)
    a_f, a_d = (act_terms(s, act) if act == "hardsigmoid" else (None, None))
    if a_f is not None:
        a_f, a_d = a_f.reshape(r.gate.shape), a_d.reshape(r.gate.shape)
    t_gate = act_tol32(r.gate, act, "fwd", a_f)
    t_dgate = act_tol32(r.dgate, act, "bwd", a_d)
    rep = {}
    if y is not None:
        rep["y"] = ratio(y, r.y, out_round(r.y, dtype) + xd.abs() * t_gate
                         + gamma(1) * r.y.abs())
    if gx is not None:
        rep["gx"] = ratio(gx, r.gx, out_round(r.gx, dtype) + gd.abs() * t_gate
                          + gamma(1) * r.gx.abs())
    if gs is not None:
        # hw products summed in any order, then the product with gate'
        rep["gs"] = ratio(d64(gs).reshape(r.gs.shape), r.gs,
                          out_round(r.gs, dtype)
                          + gamma(r.hw + 2) * r.dot_abs * r.dgate.abs()
                          + (r.dot_abs * (1 + gamma(r.hw))) * t_dgate)
    return rep


def check_maxpool(y, gx, x, g, k, stride, pad, dtype):
    yr, gxr, gabs = maxpool(x, g, k, stride, pad)
    rep = {}
    if y is not None:
        rep["n_y"] = int((d64(y) != yr).sum())  # a max is exact
    if gx is not None:
        rep["gx"] = ratio(gx, gxr, pool_bound(gxr, gabs, k, dtype))
    return rep


def check_avgpool(y, gx, x, g, k, stride, pad, dtype):
    yr, gxr, ya, gxa = avgpool(x, g, k, stride, pad)
    rep = {}
    if y is not None:
        rep["y"] = ratio(y, yr, pool_bound(yr, ya, k, dtype))
    if gx is not None:
        rep["gx"] = ratio(gx, gxr, pool_bound(gxr, gxa, k, dtype))
    return rep


def check_xent(loss, softmax, grad, logits, target, scale, dtype):
    r = softmax_xent(logits, target, scale, dtype)
    rep = {}
    if loss is not None:
        rep["loss"] = ratio(d64(loss).reshape(()), r.loss, r.b_loss)
    if softmax is not None:
        rep["softmax"] = ratio(softmax, r.p, r.b_p)
    if grad is not None:
        rep["grad"] = ratio(grad, r.grad, r.b_grad)
    return rep
