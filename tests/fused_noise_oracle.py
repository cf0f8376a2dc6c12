"""fp64 oracle for the fused noisy conv / linear kernels.

    out = conv(x, wq) + bias + N(0, sqrt(factor * conv(x, f(|w_raw|))))

A plain helper module (CPU tensors only) shared by test_fused_noise_oracle.py,
which proves on the CPU that the checks below can fail, and by the GPU tests.

Every output is handled as an [M, K] matrix: row m = (n, oh, ow) in row-major
order, column k = output channel. That is the kernels' own index space: the
Philox counter is m*K + k and one gauss4 draw covers rows m..m+3 (m % 4 == 0)
of one column, which is why the statistics below look along m in steps of 1..4
and at the residue classes m mod 4.
"""

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

# relative rounding allowance of the output dtype: the largest relative
# error of one round-to-nearest in bf16 (8 significand bits), and one ulp
# in fp16 and fp32
U_OUT = {
    torch.bfloat16: 2.0 ** -8,
    torch.float16: 2.0 ** -10,
    torch.float32: 2.0 ** -23,
}

N_SE = 5.0  # every statistic must lie within this many standard errors


def gamma(n):
    """Summation bound for an fp32-accumulated contraction of length n (n
    also counts partial sums where a kernel adds slabs). The standard bound
    is (n+1) * 2^-24 relative to sum|a||b|; the factor 2 is there because the
    MFMA's internal add order and rounding are not documented per add."""
    return 2.0 * (n + 1) * 2.0 ** -24


def sigma_weight(w_raw64, mode):
    aw = w_raw64.abs()
    return aw * aw + aw if mode == "abs2" else aw


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def _round(t, dtype):
    return t.to(dtype)


def _weights(shape, std, dtype, gen):
    w = torch.randn(shape, generator=gen) * std
    if dtype == torch.float16:
        # no fp16-subnormal operands (|w| >= 2^-10 >> 2^-14)
        w = torch.where(w < 0, -w.abs().clamp_min(2.0 ** -10),
                        w.abs().clamp_min(2.0 ** -10))
    return _round(w, dtype)


def make_inputs(x_shape, w_shape, dtype, seed, signed_x=False):
    """x on the 4-bit grid randint(0,16)/15 (or randn when signed_x),
    wq ~ 0.2 randn, w_raw ~ 0.05 randn, bias ~ 0.5 randn, all rounded to
    ``dtype``. The 4x scale gap between wq and w_raw turns a mix-up of the
    two into a z-score deviation of 2 instead of about 1."""
    gen = torch.Generator().manual_seed(seed)
    if signed_x:
        x = torch.randn(x_shape, generator=gen)
    else:
        x = torch.randint(0, 16, x_shape, generator=gen).float() / 15.0
    return SimpleNamespace(
        x=_round(x, dtype),
        wq=_weights(w_shape, 0.2, dtype, gen),
        w_raw=_weights(w_shape, 0.05, dtype, gen),
        bias=_round(torch.randn(w_shape[0], generator=gen) * 0.5, dtype),
    )


# ---------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------


def to_mk(t):
    """[N,K,OH,OW] (any memory format) or [M,K] -> fp64 [M, K] on the CPU."""
    t = t.detach().cpu().double()
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.contiguous()


def conv_refs(x, wq, w_raw, bias, stride, pad, mode):
    """fp64 references of one fused noisy conv, each as an [M, K] matrix.

    clean = conv(x, wq) + bias          sig     = conv(x, f(|w_raw|))
    sig_abs = conv(x, |w_raw|)          A       = conv(|x|, |wq|) + |bias|
    sig_mag = conv(|x|, f(|w_raw|))     n       = contraction length
    ``bias`` may be None."""
    x, wq, w_raw = x.double(), wq.double(), w_raw.double()
    b = None if bias is None else bias.double()

    def conv(a, w, bb=None):
        return to_mk(F.conv2d(a, w, bb, stride, pad))

    fw = sigma_weight(w_raw, mode)
    return SimpleNamespace(
        clean=conv(x, wq, b),
        sig=conv(x, fw),
        sig_abs=conv(x, w_raw.abs()),
        A=conv(x.abs(), wq.abs(), None if b is None else b.abs()),
        sig_mag=conv(x.abs(), fw),
        n=wq.shape[1] * wq.shape[2] * wq.shape[3],
    )


def linear_refs(x, wq, w_raw, bias, mode):
    x, wq, w_raw = x.double(), wq.double(), w_raw.double()
    b = None if bias is None else bias.double()
    fw = sigma_weight(w_raw, mode)
    return SimpleNamespace(
        clean=F.linear(x, wq, b),
        sig=F.linear(x, fw),
        sig_abs=F.linear(x, w_raw.abs()),
        A=F.linear(x.abs(), wq.abs(), None if b is None else b.abs()),
        sig_mag=F.linear(x.abs(), fw),
        n=wq.shape[1],
    )


# ---------------------------------------------------------------------------
# deterministic bound
# ---------------------------------------------------------------------------


def det_bound(ref, A, n, dtype):
    """|got - ref| <= u_out*|ref| + gamma(n)*A for an fp32-accumulated result
    rounded once to ``dtype``."""
    return U_OUT[dtype] * ref.abs() + gamma(n) * A


def bound_ratio(got, ref, bound):
    """max |got-ref| / bound (0/0 counts as 0: exact where the bound is 0)."""
    err = (to_mk(got) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return float(ratio.max())


def assert_within(got, ref, bound, what):
    r = bound_ratio(got, ref, bound)
    print("%s: worst |err|/bound = %.3g" % (what, r))
    assert r <= 1.0, "%s: |err| reaches %.3g x the derived bound" % (what, r)
    return r


# ---------------------------------------------------------------------------
# statistical check of the noise field
# ---------------------------------------------------------------------------


def _std_dev(z, valid, dim=None):
    """(sample std, count) of the valid entries, overall or along ``dim``."""
    if dim is None:
        n = valid.sum()
        mean = (z * valid).sum() / n
        var = (((z - mean) ** 2) * valid).sum() / n
    else:
        n = valid.sum(dim)
        mean = (z * valid).sum(dim) / n
        var = (((z - mean.unsqueeze(dim)) ** 2) * valid).sum(dim) / n
    return var.sqrt(), n


def _autocorr(zc, valid, var, lag, axis):
    a = zc.narrow(axis, 0, zc.shape[axis] - lag)
    b = zc.narrow(axis, lag, zc.shape[axis] - lag)
    both = valid.narrow(axis, 0, zc.shape[axis] - lag) \
        * valid.narrow(axis, lag, zc.shape[axis] - lag)
    pairs = both.sum()
    r = (a * b * both).sum() / pairs / var
    return float(r), float(pairs)


def noise_field_report(out, clean, sig, factor, stats=None, mask=None):
    """Deviation of every statistic of z = (out-clean)/sqrt(factor*sig) from
    its value under iid N(0,1), in units of its own standard error (computed
    from the number of z-scores that enter it). Group statistics report the
    worst group. ``mask`` ([M,K] bool) narrows the elements used further.
    Returns (report dict, fraction of elements used)."""
    out, clean, sig = to_mk(out), to_mk(clean), to_mk(sig)
    # elements whose sigma is ~0 carry no noise to test
    floor = 1e-6 * float(sig.abs().mean())
    validb = sig > floor
    if mask is not None:
        validb = validb & mask
    valid = validb.double()
    z = torch.where(validb, (out - clean)
                    / (factor * sig.clamp_min(floor)).sqrt(),
                    torch.zeros_like(out))
    n = float(valid.sum())
    mean = float((z * valid).sum() / n)
    zc = (z - mean) * valid
    var = float((zc ** 2).sum() / n)
    rep = {}
    rep["mean"] = abs(mean) / (1.0 / math.sqrt(n))
    rep["std"] = abs(math.sqrt(var) - 1.0) / (1.0 / math.sqrt(2.0 * n))
    kurt = float((zc ** 4).sum() / n) / var ** 2 - 3.0
    rep["kurtosis"] = abs(kurt) / math.sqrt(24.0 / n)
    for lag in (1, 2, 3, 4):
        r, pairs = _autocorr(zc, valid, var, lag, 0)
        rep["lag%d_m" % lag] = abs(r) * math.sqrt(pairs)
    r, pairs = _autocorr(zc, valid, var, 1, 1)
    rep["lag1_k"] = abs(r) * math.sqrt(pairs)
    # every output channel on its own
    sd, cnt = _std_dev(z, valid, dim=0)
    rep["channel_std"] = float(((sd - 1.0).abs() * (2.0 * cnt).sqrt()).max())
    cmean = (z * valid).sum(0) / cnt
    rep["channel_mean"] = float((cmean.abs() * cnt.sqrt()).max())
    # every residue class m mod 4 (the four rows of one gauss4 draw)
    worst = 0.0
    for res in range(4):
        sd, cnt = _std_dev(z[res::4], valid[res::4])
        worst = max(worst, float((sd - 1.0).abs() * (2.0 * cnt).sqrt()))
    rep["mod4_std"] = worst
    if stats is not None:
        rep = {k: rep[k] for k in stats}
    return rep, n / z.numel()


def check_noise_field(out, clean, sig, factor, stats=None, what="noise field",
                      mask=None, min_used=0.99):
    """Assert that ``out - clean`` is iid N(0, factor*sig): every statistic of
    noise_field_report within N_SE standard errors, on at least 99 % of the
    elements. ``stats`` restricts the check to the named statistics; ``mask``
    and ``min_used`` serve inputs whose sigma is not positive everywhere."""
    rep, used = noise_field_report(out, clean, sig, factor, stats, mask)
    print("%s: used %.4f, " % (what, used)
          + ", ".join("%s %.2f" % kv for kv in rep.items()) + " (SE)")
    assert used >= min_used, "%s: only %.3f of the elements have sigma > 0" % (
        what, used)
    bad = {k: round(v, 1) for k, v in rep.items() if not v <= N_SE}
    assert not bad, "%s: beyond %g standard errors: %s" % (what, N_SE, bad)
    return rep
