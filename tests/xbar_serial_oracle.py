"""fp64 oracle of the tiled-crossbar ops with bit-serial inputs
(ops.xbar_noisy_conv2d / _linear with dac_bits > 0).

The activation is a B-bit code on the grid x_step and reaches the rows D bits
per cycle, J = ceil(B / D) slices. With the noise off, per block b (rows as in
xbar_oracle) and slice j

    code = clamp(rint(f32(x) * inv_x_step), 0, 2^B - 1)
    d_j  = (code >> j*D) & (2^D - 1)
    p_bj = x_step * sum_{k in b} d_j,k * wq_k
    q_bj = step * clamp(rint(p_bj / step), -Qm, Qm)
    out  = sum_b sum_j 2^(jD) q_bj + bias

``x_step`` and ``inv_x_step`` are the fp32 numbers the op computes (x_step
rounded once to fp32 and one fp32 division), and the code is derived with
exactly the op's fp32 product; ``step`` as in xbar_oracle. Everything else is
fp64 on CPU tensors, [M, K] matrices in the index space of fused_noise_oracle.

A plain helper module shared by test_xbar_serial_oracle.py (CPU) and
test_xbar_serial_gpu.py.
"""

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

import fused_noise_oracle as fo
import xbar_oracle as xo

gamma, U_OUT = fo.gamma, fo.U_OUT


def dac_step(x_step):
    """(x_step, 1/x_step) as the op uses them: fp32, one division."""
    xs = np.float32(x_step)
    return float(xs), float(np.float32(1.0) / xs)


def codes(xm, x_step, in_bits):
    """Integer codes (int64) of a row matrix, by the op's own fp32 product."""
    _, inv = dac_step(x_step)
    c = torch.round(xm.float() * torch.tensor(inv, dtype=torch.float32))
    return c.clamp(0, float(2 ** in_bits - 1)).to(torch.int64)


def blocked(xm, wqm, wrm, bias, mode, xbar_rows, adc_bits, adc_max, x_step,
            in_bits, dac_bits):
    """Sliced blocked reference on row matrices xm [M, n], wqm / wrm [K, n].

    Lists hold one [M, K] fp64 tensor per (b, j), b ascending and j ascending
    inside b; ``shift`` holds the matching 2^(jD):
      t      p_bj / step (p_bj itself with the ADC off)
      A      x_step * sum d_j |wq|
      s      max(x_step * sum d_j f(|w_raw|), 0)   (None without ``mode``)
      s_abs  x_step * sum d_j |w_raw|              (None without ``mode``)
    and out (shift-added, noise off), clean (sum 2^(jD) p_bj + bias), qabs
    (sum 2^(jD) |q_bj|), clipped (count of |rint(t)| > Qm over all (b, j)),
    absmax (max |p_bj|), code (the [M, n] integer codes), J, nblocks, n."""
    D, B = int(dac_bits), int(in_bits)
    J = -(-B // D)
    xs, _ = dac_step(x_step)
    code = codes(xm, x_step, B)
    wqm = wqm.double()
    n = xm.shape[1]
    adc = adc_bits > 0
    step, qm = xo.adc_step(adc_bits, adc_max) if adc else (1.0, float("inf"))
    fw = aw = None
    if mode is not None:
        aw = wrm.double().abs()
        fw = fo.sigma_weight(wrm.double(), mode)
    out = torch.zeros(xm.shape[0], wqm.shape[0], dtype=torch.float64)
    clean, qabs = out.clone(), out.clone()
    ts, As, ss, sabs, shifts = [], [], [], [], []
    clipped, absmax, nblocks = 0, 0.0, 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        nblocks += 1
        for j in range(J):
            shift = float(2 ** (j * D))
            dj = ((code[:, k0:k1] >> (j * D)) & (2 ** D - 1)).double()
            p = xs * (dj @ wqm[:, k0:k1].t())
            t = p / step
            if adc:
                r = torch.round(t)                     # half to even
                clipped += int((r.abs() > qm).sum())
                q = step * r.clamp(-qm, qm)
            else:
                q = p
            out += shift * q
            clean += shift * p
            qabs += shift * q.abs()
            absmax = max(absmax, float(p.abs().max()))
            ts.append(t)
            shifts.append(shift)
            As.append(xs * (dj @ wqm[:, k0:k1].abs().t()))
            if mode is not None:
                ss.append((xs * (dj @ fw[:, k0:k1].t())).clamp_min(0))
                sabs.append(xs * (dj @ aw[:, k0:k1].t()))
    if bias is not None:
        out += bias.double()
        clean += bias.double()
    return SimpleNamespace(
        out=out, clean=clean, t=ts, A=As, shift=shifts,
        s=ss if mode else None, s_abs=sabs if mode else None, qabs=qabs,
        step=step, qm=qm, x_step=xs, J=J, D=D, nblocks=nblocks, n=n,
        clipped=clipped, absmax=absmax, code=code,
        n_partials=J * nblocks * out.numel(),
        bias_abs=(torch.zeros(wqm.shape[0], dtype=torch.float64)
                  if bias is None else bias.double().abs()))


def conv_blocked(x, wq, w_raw, bias, stride, pad, mode, xbar_rows, adc_bits,
                 adc_max, x_step, in_bits, dac_bits):
    R, S = wq.shape[2], wq.shape[3]
    return blocked(xo.conv_rows(x, R, S, stride, pad), xo.weight_rows(wq),
                   None if w_raw is None else xo.weight_rows(w_raw), bias,
                   mode, xbar_rows, adc_bits, adc_max, x_step, in_bits,
                   dac_bits)


def linear_blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max,
                   x_step, in_bits, dac_bits):
    return blocked(x, wq, w_raw, bias, mode, xbar_rows, adc_bits, adc_max,
                   x_step, in_bits, dac_bits)


def noise_variance(ref):
    """sum_bj 4^(jD) s_bj: the shift-added output noise variance / factor."""
    return sum(sh * sh * s for sh, s in zip(ref.shift, ref.s))


# ---------------------------------------------------------------------------
# the noise-off, ADC-on comparison for general inputs
# ---------------------------------------------------------------------------


def adc_report(got, ref, xbar_rows, dtype):
    """Compare a kernel result with the ADC on and the noise off.

    A slice partial is *flagged* when t_bj = p_bj/step is so close to a
    rounding boundary that an fp32 evaluation may land on the other side:
        |frac(t) - 0.5| <= gamma(xbar_rows) * A_bj / step + 2^-21 (|t| + 1)
    (summation error of the block; the fp32 roundings of step, 1/step and the
    product as in xbar_oracle, and one bit more for the x_step multiply).
    Outputs with no flagged partial must satisfy
        |out - oracle| <= (U_OUT + gamma(J*nblocks + 1)) * (sum 2^(jD)|q_bj| + |bias|)
    (the digital shift-add of J*nblocks exact-valued partials plus bias,
    rounded once to the dtype); a flagged partial adds 2^(jD) * step.
    Returns (excluded share, worst |err| / bound)."""
    got = fo.to_mk(got)
    flags = torch.zeros_like(ref.out)
    extra = torch.zeros_like(ref.out)
    for t, A, sh in zip(ref.t, ref.A, ref.shift):
        frac = t - torch.floor(t)
        slack = gamma(xbar_rows) * A / ref.step + 2.0 ** -21 * (t.abs() + 1)
        f = ((frac - 0.5).abs() <= slack).double()
        flags += f
        extra += sh * ref.step * f
    bound = (U_OUT[dtype] + gamma(ref.J * ref.nblocks + 1)) \
        * (ref.qabs + ref.bias_abs) + extra
    err = (got - ref.out).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return float((flags > 0).double().mean()), float(ratio.max())


def assert_adc_close(got, ref, xbar_rows, dtype, what, max_excluded=0.05):
    excluded, worst = adc_report(got, ref, xbar_rows, dtype)
    print("%s: excluded %.4f, worst |err|/bound %.3g, clip share %.4f" % (
        what, excluded, worst, ref.clipped / float(ref.n_partials)))
    assert excluded <= max_excluded, "%s: %.3f of the outputs sit on a " \
        "rounding boundary" % (what, excluded)
    assert worst <= 1.0, "%s: |err| reaches %.3g x the bound" % (what, worst)


# ---------------------------------------------------------------------------
# the shapes, inputs and configurations shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------

# name -> (kind, x shape, w shape, stride, pad): the shapes of test_xbar_gpu,
# the smallest that cross every boundary of the 64x64x32 tile
SHAPES = {
    "linear": ("linear", (130, 296), (80, 296), 1, 0),
    "convA": ("conv", (3, 5, 9, 9), (70, 5, 5, 5), 2, 2),
    "convB": ("conv", (3, 32, 6, 6), (20, 32, 3, 3), 1, 1),
}
# (xbar_rows, adc_bits, adc_max, dac_bits). Exact inputs: x_step 1, B = 4,
# power-of-two steps 1, 2, 0.5 and 8; the last one is a single slice
EXACT_CFGS = [(128, 4, 7.0, 1), (64, 4, 14.0, 2), (32, 4, 3.5, 1),
              (64, 4, 56.0, 4)]
# General inputs (fo.make_inputs, on the 4-bit grid): x_step 1/15, B = 4
GENERAL_CFGS = {
    "linear": [(128, 5, 0.25, 1), (64, 4, 0.5, 2), (32, 6, 0.125, 1),
               (64, 5, 2.0, 4)],
    "convA": [(64, 5, 0.15, 1), (32, 4, 0.25, 2)],
}
IN_BITS = 4
X_STEP = {"exact": 1.0, "general": 1.0 / 15.0}


@lru_cache(maxsize=None)
def general_inputs(shape, dtype, seed=1, batch=None):
    kind, xs, ws, stride, pad = SHAPES[shape]
    if batch is not None:
        xs = (batch,) + xs[1:]
    return fo.make_inputs(xs, ws, dtype, seed)


@lru_cache(maxsize=None)
def exact_inputs(shape, dtype):
    """Integer-grid inputs (those of test_xbar_gpu): x = randint(0,16), wq and
    w_raw = randint(-8,9)/8, bias a multiple of 1/8. With x_step = 1 and a
    power-of-two step every product, partial sum and v/step is exact in fp32
    in any order."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    gen = torch.Generator().manual_seed(17)
    return SimpleNamespace(
        x=torch.randint(0, 16, xs, generator=gen).float().to(dtype),
        wq=(torch.randint(-8, 9, ws, generator=gen).float() / 8).to(dtype),
        w_raw=(torch.randint(-8, 9, ws, generator=gen).float() / 8).to(dtype),
        bias=(torch.randint(-8, 9, (ws[0],), generator=gen).float() / 8).to(dtype))


@lru_cache(maxsize=None)
def oracle(shape, dtype, inputs, mode, rows, bits, amax, dac_bits, bias=True,
           batch=None):
    kind, xs, ws, stride, pad = SHAPES[shape]
    inp = exact_inputs(shape, dtype) if inputs == "exact" \
        else general_inputs(shape, dtype, batch=batch)
    b = inp.bias if bias else None
    if kind == "conv":
        return conv_blocked(inp.x, inp.wq, inp.w_raw, b, stride, pad, mode,
                            rows, bits, amax, X_STEP[inputs], IN_BITS,
                            dac_bits)
    return linear_blocked(inp.x, inp.wq, inp.w_raw, b, mode, rows, bits, amax,
                          X_STEP[inputs], IN_BITS, dac_bits)


def tie_share(ref):
    return sum(float(((t - torch.floor(t)) == 0.5).double().mean())
               for t in ref.t) / len(ref.t)


def clip_share(ref):
    return ref.clipped / float(ref.n_partials)
