"""fp64 oracle of the tiled-crossbar ops (ops.xbar_noisy_conv2d / _linear).

The contraction index ("crossbar row") of a conv is the filter's memory order
(r, s, c), c fastest; of a linear layer the input index. Block b is rows
[b*xbar_rows, min((b+1)*xbar_rows, n)). Per block, with the noise off,

    p_b = sum_{k in b} x_k * wq_k
    q_b = step * clamp(rint(p_b / step), -Qm, Qm)     Qm = 2^(bits-1) - 1
    out = sum_b q_b + bias                            step = adc_max / Qm

``step`` is the fp32 number the op computes (adc_max / Qm rounded once to
fp32); everything else here is fp64 on CPU tensors. Outputs are [M, K]
matrices in the index space of fused_noise_oracle (row m = (n, oh, ow)).

A plain helper module shared by test_xbar_oracle.py (CPU) and
test_xbar_gpu.py.
"""

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import fused_noise_oracle as fo

gamma, U_OUT, N_SE = fo.gamma, fo.U_OUT, fo.N_SE


def adc_step(adc_bits, adc_max):
    """(step, Qm) as the op uses them: step is one fp32 division."""
    qm = 2 ** (adc_bits - 1) - 1
    return float(np.float32(adc_max) / np.float32(qm)), float(qm)


def conv_rows(x, R, S, stride, pad, order="rsc"):
    """im2col matrix [M, R*S*C] of an NCHW tensor, fp64; padding rows are 0.
    order 'rsc' is the crossbar row order, 'crs' the NCHW filter order."""
    x = x.double()
    N, C, H, W = x.shape
    oh = (H + 2 * pad - R) // stride + 1
    ow = (W + 2 * pad - S) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    taps = []
    for r in range(R):
        for s in range(S):
            patch = xp[:, :, r:r + stride * (oh - 1) + 1:stride,
                       s:s + stride * (ow - 1) + 1:stride]
            taps.append(patch.permute(0, 2, 3, 1).reshape(N * oh * ow, C))
    rows = torch.stack(taps, 1)                       # [M, R*S, C]
    if order == "crs":
        rows = rows.permute(0, 2, 1)
    return rows.reshape(rows.shape[0], -1).contiguous()


def weight_rows(w, order="rsc"):
    w = w.double()
    if w.dim() == 2:
        return w
    if order == "rsc":
        w = w.permute(0, 2, 3, 1)
    return w.reshape(w.shape[0], -1).contiguous()


def blocked(xm, wqm, wrm, bias, mode, xbar_rows, adc_bits, adc_max):
    """Blocked reference on fp64 row matrices xm [M, n], wqm / wrm [K, n].

    Returns a namespace of [M, K] fp64 tensors (lists hold one per block):
      out    sum_b q_b + bias with the noise off
      clean  sum_b p_b + bias (the unblocked result)
      t      [p_b / step]   (p_b itself with the ADC off)
      A      [sum |x||wq|]  per block
      s      [max(sum x f(|w_raw|), 0)] per block (None without ``mode``)
      s_abs  [sum x |w_raw|] per block (None without ``mode``)
      qabs   sum_b |q_b|
    and step, qm, nblocks, n, clipped (count of |rint(t_b)| > Qm) and absmax
    (max |p_b|)."""
    xm, wqm = xm.double(), wqm.double()
    n = xm.shape[1]
    adc = adc_bits > 0
    step, qm = adc_step(adc_bits, adc_max) if adc else (1.0, float("inf"))
    fw = aw = None
    if mode is not None:
        aw = wrm.double().abs()
        fw = fo.sigma_weight(wrm.double(), mode)
    out = torch.zeros(xm.shape[0], wqm.shape[0], dtype=torch.float64)
    clean, qabs = out.clone(), out.clone()
    ts, As, ss, sabs = [], [], [], []
    clipped, absmax = 0, 0.0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        p = xb @ wqm[:, k0:k1].t()
        t = p / step
        if adc:
            r = torch.round(t)                     # half to even
            clipped += int((r.abs() > qm).sum())
            q = step * r.clamp(-qm, qm)
        else:
            q = p
        out += q
        clean += p
        qabs += q.abs()
        absmax = max(absmax, float(p.abs().max()))
        ts.append(t)
        As.append(xb.abs() @ wqm[:, k0:k1].abs().t())
        if mode is not None:
            ss.append((xb @ fw[:, k0:k1].t()).clamp_min(0))
            sabs.append(xb @ aw[:, k0:k1].t())
    if bias is not None:
        out += bias.double()
        clean += bias.double()
    return SimpleNamespace(
        out=out, clean=clean, t=ts, A=As, s=ss if mode else None,
        s_abs=sabs if mode else None, qabs=qabs, step=step, qm=qm,
        nblocks=len(ts), n=n, clipped=clipped, absmax=absmax,
        bias_abs=(torch.zeros(wqm.shape[0], dtype=torch.float64)
                  if bias is None else bias.double().abs()))


def conv_blocked(x, wq, w_raw, bias, stride, pad, mode, xbar_rows, adc_bits,
                 adc_max, order="rsc"):
    R, S = wq.shape[2], wq.shape[3]
    return blocked(conv_rows(x, R, S, stride, pad, order),
                   weight_rows(wq, order),
                   None if w_raw is None else weight_rows(w_raw, order),
                   bias, mode, xbar_rows, adc_bits, adc_max)


def linear_blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max):
    return blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max)


# ---------------------------------------------------------------------------
# the noise-off, ADC-on comparison for general inputs
# ---------------------------------------------------------------------------


def adc_report(got, ref, xbar_rows, dtype):
    """Compare a kernel result with the ADC on and the noise off.

    A block partial is *flagged* when its t_b = p_b/step is so close to a
    rounding boundary that an fp32 accumulation may land on the other side:
        |frac(t_b) - 0.5| <= gamma(xbar_rows) * A_b / step + 2^-22 (|t_b| + 1)
    (summation error of the block, plus the fp32 rounding of step, 1/step and
    the product). Outputs with no flagged block must satisfy
        |out - oracle| <= (U_OUT + gamma(nblocks + 1)) * (sum_b |q_b| + |bias|)
    (the digital sum of nblocks exact-valued partials plus bias, rounded once
    to the dtype); outputs with flagged blocks get ``step`` more per flag.
    Returns (excluded share, worst |err| / bound)."""
    got = fo.to_mk(got)
    flags = torch.zeros_like(ref.out)
    for t, A in zip(ref.t, ref.A):
        frac = t - torch.floor(t)
        slack = gamma(xbar_rows) * A / ref.step + 2.0 ** -22 * (t.abs() + 1)
        flags += ((frac - 0.5).abs() <= slack).double()
    bound = (U_OUT[dtype] + gamma(ref.nblocks + 1)) * (ref.qabs + ref.bias_abs) \
        + ref.step * flags
    err = (got - ref.out).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return float((flags > 0).double().mean()), float(ratio.max())


def assert_adc_close(got, ref, xbar_rows, dtype, what, max_excluded=0.05):
    excluded, worst = adc_report(got, ref, xbar_rows, dtype)
    print("%s: excluded %.4f, worst |err|/bound %.3g, clip share %.4f" % (
        what, excluded, worst,
        ref.clipped / float(ref.nblocks * ref.out.numel())))
    assert excluded <= max_excluded, "%s: %.3f of the outputs sit on a " \
        "rounding boundary" % (what, excluded)
    assert worst <= 1.0, "%s: |err| reaches %.3g x the bound" % (what, worst)
