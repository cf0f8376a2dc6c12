"""fp64 oracle of the tiled-crossbar ops on differential columns
(ops.xbar_noisy_conv2d / _linear with ``differential=True``).

Rows, blocks and the row order are those of xbar_oracle.py. Every block runs on
two columns: the positive and the negative part of the weights, each digitised
by a unipolar ADC and subtracted digitally. Per block, with the noise off,

    wq+ = max(wq, 0)      wq- = max(-wq, 0)
    p+- = sum_{k in b} x_k * wq+-_k
    q+- = step * clamp(rint(p+- / step), 0, Qu)       Qu = 2^bits - 1
    out = sum_b (q+ - q-) + bias                      step = adc_max / Qu

``step`` is the fp32 number the op computes; everything else is fp64 on CPU
tensors. Per-column lists hold 2 * nblocks entries: block 0's positive column,
block 0's negative column, block 1's positive column, ...

A plain helper module shared by test_xbar_diff_oracle.py (CPU) and
test_xbar_diff_gpu.py.
"""

from types import SimpleNamespace

import numpy as np
import torch

import fused_noise_oracle as fo
import xbar_oracle as xo

gamma, U_OUT = fo.gamma, fo.U_OUT


def adc_step(adc_bits, adc_max):
    """(step, Qu) of the unipolar ADC: step is one fp32 division."""
    qu = 2 ** adc_bits - 1
    return float(np.float32(adc_max) / np.float32(qu)), float(qu)


def blocked(xm, wqm, wrm, bias, mode, xbar_rows, adc_bits, adc_max):
    """Differential reference on fp64 row matrices xm [M, n], wqm / wrm [K, n].

    Returns what xbar_oracle.blocked returns, per column:
      out    sum_b (q+ - q-) + bias with the noise off
      clean  sum_b (p+ - p-) + bias (the unblocked signed result)
      t      [p+- / step]   per column partial (p+- with the ADC off)
      A      [sum |x| wq+-] per column partial
      s      [max(sum x f+-, 0)] per column partial (None without ``mode``),
             f+- = f(|w_raw|) where w_raw > 0 / < 0, else 0
      s_abs  [sum x |w_raw|] per block (None without ``mode``)
      qabs   sum over the column partials of |q+-|
    and step, qu, nblocks, n, clipped (count of column partials with
    rint(t) > Qu or < 0) and absmax (max |p+-|)."""
    xm, wqm = xm.double(), wqm.double()
    n = xm.shape[1]
    adc = adc_bits > 0
    step, qu = adc_step(adc_bits, adc_max) if adc else (1.0, float("inf"))
    wqs = (wqm.clamp_min(0), (-wqm).clamp_min(0))
    fws = aw = None
    if mode is not None:
        wr = wrm.double()
        aw = wr.abs()
        fw = fo.sigma_weight(wr, mode)
        zero = torch.zeros_like(fw)
        fws = (torch.where(wr > 0, fw, zero), torch.where(wr < 0, fw, zero))
    out = torch.zeros(xm.shape[0], wqm.shape[0], dtype=torch.float64)
    clean, qabs = out.clone(), out.clone()
    ts, As, ss, sabs = [], [], [], []
    clipped, absmax, nblocks = 0, 0.0, 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        nblocks += 1
        for col, sgn in ((0, 1.0), (1, -1.0)):
            w = wqs[col][:, k0:k1]
            p = xb @ w.t()
            t = p / step
            if adc:
                r = torch.round(t)                     # half to even
                clipped += int(((r > qu) | (r < 0)).sum())
                q = step * r.clamp(0, qu)
            else:
                q = p
            out += sgn * q
            clean += sgn * p
            qabs += q.abs()
            absmax = max(absmax, float(p.abs().max()))
            ts.append(t)
            As.append(xb.abs() @ w.t())
            if mode is not None:
                ss.append((xb @ fws[col][:, k0:k1].t()).clamp_min(0))
        if mode is not None:
            sabs.append(xb @ aw[:, k0:k1].t())
    if bias is not None:
        out += bias.double()
        clean += bias.double()
    return SimpleNamespace(
        out=out, clean=clean, t=ts, A=As, s=ss if mode else None,
        s_abs=sabs if mode else None, qabs=qabs, step=step, qu=qu,
        nblocks=nblocks, n=n, clipped=clipped, absmax=absmax,
        n_partials=2 * nblocks * out.numel(),
        bias_abs=(torch.zeros(wqm.shape[0], dtype=torch.float64)
                  if bias is None else bias.double().abs()))


def conv_blocked(x, wq, w_raw, bias, stride, pad, mode, xbar_rows, adc_bits,
                 adc_max):
    R, S = wq.shape[2], wq.shape[3]
    return blocked(xo.conv_rows(x, R, S, stride, pad),
                   xo.weight_rows(wq),
                   None if w_raw is None else xo.weight_rows(w_raw),
                   bias, mode, xbar_rows, adc_bits, adc_max)


def linear_blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max):
    return blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max)


def clip_share(ref):
    return ref.clipped / float(ref.n_partials)


def tie_share(ref):
    """Share of the column partials whose t sits exactly on a rounding tie."""
    return sum(float(((t - torch.floor(t)) == 0.5).double().mean())
               for t in ref.t) / len(ref.t)


# ---------------------------------------------------------------------------
# the noise-off, ADC-on comparison for general inputs
# ---------------------------------------------------------------------------


def adc_report(got, ref, xbar_rows, dtype):
    """The flag-and-bound scheme of xbar_oracle.adc_report, per column partial.

    A column partial is *flagged* when
        |frac(t) - 0.5| <= gamma(xbar_rows) * A / step + 2^-22 (|t| + 1).
    Outputs with no flagged partial must satisfy
        |out - oracle| <= (U_OUT + gamma(2 nblocks + 1)) * (sum |q+-| + |bias|)
    (the digital sum of 2 nblocks exact-valued column codes plus bias, rounded
    once to the dtype); outputs with flagged partials get ``step`` more per
    flag. Returns (share of outputs with a flag, worst |err| / bound)."""
    got = fo.to_mk(got)
    flags = torch.zeros_like(ref.out)
    for t, A in zip(ref.t, ref.A):
        frac = t - torch.floor(t)
        slack = gamma(xbar_rows) * A / ref.step + 2.0 ** -22 * (t.abs() + 1)
        flags += ((frac - 0.5).abs() <= slack).double()
    bound = (U_OUT[dtype] + gamma(2 * ref.nblocks + 1)) \
        * (ref.qabs + ref.bias_abs) + ref.step * flags
    err = (got - ref.out).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return float((flags > 0).double().mean()), float(ratio.max())


def assert_adc_close(got, ref, xbar_rows, dtype, what, max_excluded=0.05):
    excluded, worst = adc_report(got, ref, xbar_rows, dtype)
    print("%s: excluded %.4f, worst |err|/bound %.3g, column clip share %.4f"
          % (what, excluded, worst, clip_share(ref)))
    assert excluded <= max_excluded, "%s: %.3f of the outputs sit on a " \
        "rounding boundary" % (what, excluded)
    assert worst <= 1.0, "%s: |err| reaches %.3g x the bound" % (what, worst)
