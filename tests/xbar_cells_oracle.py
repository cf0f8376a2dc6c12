"""fp64 oracle of the tiled-crossbar ops with bit-sliced weights
(ops.xbar_noisy_conv2d / _linear with cell_bits > 0).

A cell holds E bits, so the B-bit offset-binary code of a weight on the grid
w = w_min + code * w_step is spread over T = ceil(B / E) columns. With the
noise off, per block b (rows as in xbar_oracle) and slice t

    code = clamp(rint((f32(wq) - w_min) * inv_w_step), 0, 2^B - 1)
    d_t  = (code >> t*E) & (2^E - 1)
    p_bt = w_step * sum_{k in b} x_k * d_t,k
    q_bt = step * clamp(rint(p_bt / step), 0, Qu)        Qu = 2^bits - 1
    X_b  = sum_{k in b} x_k
    out  = sum_b (sum_t 2^(tE) q_bt + w_min * X_b) + bias

``w_step``, ``inv_w_step`` and ``w_min`` are the fp32 numbers the op computes
(each rounded once to fp32, one fp32 division), and the code is derived with
exactly the op's fp32 expression; ``step`` = adc_max / Qu is one fp32 division
(the unipolar step of xbar_diff_oracle). Everything else is fp64 on CPU
tensors, [M, K] matrices in the index space of fused_noise_oracle.

A plain helper module shared by test_xbar_cells_oracle.py (CPU) and
test_xbar_cells_gpu.py.
"""

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

import fused_noise_oracle as fo
import xbar_oracle as xo
import xbar_serial_oracle as xso
from noisynet_amd.ops import reference as ref_ops

gamma, U_OUT = fo.gamma, fo.U_OUT
SHAPES = xso.SHAPES


def cell_params(w_step, w_min):
    """(w_step, 1/w_step, w_min) as the op uses them: fp32, one division."""
    ws = np.float32(w_step)
    return float(ws), float(np.float32(1.0) / ws), float(np.float32(w_min))


def adc_step(adc_bits, adc_max):
    """(step, Qu) of the unipolar column ADC: step is one fp32 division."""
    qu = 2 ** adc_bits - 1
    return float(np.float32(adc_max) / np.float32(qu)), float(qu)


def grid_step(w_bits, lo, hi):
    """The weight quantiser's LSB for the range (lo, hi)."""
    return max((hi - lo) / (2.0 ** w_bits - 1.0), 1e-6)


def codes(wqm, w_step, w_min, w_bits):
    """Integer codes (int64) of a weight matrix, by the op's own fp32
    expression."""
    _, inv, wm = cell_params(w_step, w_min)
    c = torch.round((wqm.float() - torch.tensor(wm, dtype=torch.float32))
                    * torch.tensor(inv, dtype=torch.float32))
    return c.clamp(0, float(2 ** w_bits - 1)).to(torch.int64)


def blocked(xm, wqm, bias, mode, xbar_rows, adc_bits, adc_max, w_step, w_min,
            w_bits, cell_bits):
    """Sliced blocked reference on row matrices xm [M, n], wqm [K, n].

    Lists hold one [M, K] fp64 tensor per (b, t), b ascending and t ascending
    inside b; ``shift`` holds the matching 2^(tE):
      t      p_bt / step (p_bt itself with the ADC off)
      A      p_bt for |x| (= p_bt for x >= 0)
      s      max(sum x f(w_step d_t), 0)      (None without ``mode``)
    and out (shift-added with the offset, noise off), clean (sum 2^(tE) p_bt
    + w_min X_b + bias), qabs (sum 2^(tE) |q_bt|), xabs (sum_b |X_b|, [M, 1]),
    p_sum (sum_bt of every p_bt: the cell current), clipped (count of
    rint(t) > Qu or < 0 over all (b, t)), absmax (max |p_bt|), code ([K, n]),
    w_grid (w_min + code * w_step), T, nblocks, n."""
    E, B = int(cell_bits), int(w_bits)
    T = -(-B // E)
    ws, _, wm = cell_params(w_step, w_min)
    code = codes(wqm, w_step, w_min, B)
    xm = xm.double()
    n = xm.shape[1]
    adc = adc_bits > 0
    step, qu = adc_step(adc_bits, adc_max) if adc else (1.0, float("inf"))
    out = torch.zeros(xm.shape[0], wqm.shape[0], dtype=torch.float64)
    clean, qabs = out.clone(), out.clone()
    xabs = torch.zeros(xm.shape[0], 1, dtype=torch.float64)
    ts, As, ss, shifts = [], [], [], []
    clipped, absmax, nblocks, p_sum = 0, 0.0, 0, 0.0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        nblocks += 1
        xb = xm[:, k0:k1]
        for t in range(T):
            shift = float(2 ** (t * E))
            dt = ((code[:, k0:k1] >> (t * E)) & (2 ** E - 1)).double()
            p = ws * (xb @ dt.t())
            tt = p / step
            if adc:
                r = torch.round(tt)                    # half to even
                clipped += int(((r > qu) | (r < 0)).sum())
                q = step * r.clamp(0, qu)
            else:
                q = p
            out += shift * q
            clean += shift * p
            qabs += shift * q.abs()
            absmax = max(absmax, float(p.abs().max()))
            p_sum += float(p.sum())
            ts.append(tt)
            shifts.append(shift)
            As.append(ws * (xb.abs() @ dt.t()))
            if mode is not None:
                s = p
                if mode == "abs2":
                    s = ws * ws * (xb @ (dt * dt).t()) + p
                ss.append(s.clamp_min(0))
        X = xb.sum(dim=1, keepdim=True)
        out += wm * X
        clean += wm * X
        xabs += X.abs()
    if bias is not None:
        out += bias.double()
        clean += bias.double()
    return SimpleNamespace(
        out=out, clean=clean, t=ts, A=As, shift=shifts,
        s=ss if mode else None, qabs=qabs, xabs=xabs, p_sum=p_sum, step=step,
        qu=qu, w_step=ws, w_min=wm, T=T, E=E, nblocks=nblocks, n=n,
        clipped=clipped, absmax=absmax, code=code,
        w_grid=wm + code.double() * ws,
        n_partials=T * nblocks * out.numel(),
        bias_abs=(torch.zeros(wqm.shape[0], dtype=torch.float64)
                  if bias is None else bias.double().abs()))


def conv_blocked(x, wq, bias, stride, pad, mode, xbar_rows, adc_bits, adc_max,
                 w_step, w_min, w_bits, cell_bits):
    R, S = wq.shape[2], wq.shape[3]
    return blocked(xo.conv_rows(x, R, S, stride, pad), xo.weight_rows(wq),
                   bias, mode, xbar_rows, adc_bits, adc_max, w_step, w_min,
                   w_bits, cell_bits)


def linear_blocked(x, wq, bias, mode, xbar_rows, adc_bits, adc_max, w_step,
                   w_min, w_bits, cell_bits):
    return blocked(x, wq, bias, mode, xbar_rows, adc_bits, adc_max, w_step,
                   w_min, w_bits, cell_bits)


def noise_variance(ref):
    """sum_bt 4^(tE) s_bt: the shift-added output noise variance / factor."""
    return sum(sh * sh * s for sh, s in zip(ref.shift, ref.s))


# ---------------------------------------------------------------------------
# the noise-off, ADC-on comparison for general inputs
# ---------------------------------------------------------------------------


def adc_report(got, ref, xbar_rows, dtype):
    """Compare a result with the ADC on and the noise off.

    A slice partial is *flagged* by the rule of xbar_serial_oracle.adc_report
    with A_bt = p_bt:
        |frac(t) - 0.5| <= gamma(xbar_rows) * A_bt / step + 2^-21 (|t| + 1)
    Outputs with no flagged partial must satisfy
        |out - oracle| <= (U_OUT + gamma(T*nblocks + nblocks + 1))
                          * (sum 2^(tE)|q_bt| + |w_min| sum_b |X_b| + |bias|)
    (the digital shift-add of T*nblocks exact-valued partials, nblocks offsets
    and the bias, rounded once to the dtype); a flagged partial adds
    2^(tE) * step. Returns (excluded share, worst |err| / bound)."""
    got = fo.to_mk(got)
    flags = torch.zeros_like(ref.out)
    extra = torch.zeros_like(ref.out)
    for t, A, sh in zip(ref.t, ref.A, ref.shift):
        frac = t - torch.floor(t)
        slack = gamma(xbar_rows) * A / ref.step + 2.0 ** -21 * (t.abs() + 1)
        f = ((frac - 0.5).abs() <= slack).double()
        flags += f
        extra += sh * ref.step * f
    bound = (U_OUT[dtype] + gamma(ref.T * ref.nblocks + ref.nblocks + 1)) \
        * (ref.qabs + abs(ref.w_min) * ref.xabs + ref.bias_abs) + extra
    err = (got - ref.out).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err),
                        err / bound.clamp_min(1e-300))
    return float((flags > 0).double().mean()), float(ratio.max())


def assert_adc_close(got, ref, xbar_rows, dtype, what, max_excluded=0.05):
    excluded, worst = adc_report(got, ref, xbar_rows, dtype)
    print("%s: excluded %.4f, worst |err|/bound %.3g, clip share %.4f" % (
        what, excluded, worst, clip_share(ref)))
    assert excluded <= max_excluded, "%s: %.3f of the outputs sit on a " \
        "rounding boundary" % (what, excluded)
    assert worst <= 1.0, "%s: |err| reaches %.3g x the bound" % (what, worst)


# ---------------------------------------------------------------------------
# the shapes, inputs and configurations shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------

# (xbar_rows, adc_bits, adc_max, cell_bits). Exact inputs: w_step 1,
# w_min -8, B = 4; unipolar power-of-two steps 32, 32, 8 and 128
# (adc_max = Qu * 2^k); the last one is a single slice
EXACT_CFGS = [(128, 4, 480.0, 1), (96, 5, 992.0, 2), (32, 4, 120.0, 1),
              (64, 5, 3968.0, 4)]
EXACT_W = dict(w_step=1.0, w_min=-8.0, w_bits=4)
# General inputs (fo.make_inputs, wq put on the B-bit grid over [-0.5, 0.5]):
# (xbar_rows, adc_bits, adc_max, w_bits, cell_bits)
GENERAL_CFGS = {
    "linear": [(64, 5, 1.10, 4, 1), (128, 6, 6.10, 4, 2), (32, 4, 0.30, 6, 2),
               (64, 5, 13.4, 4, 4)],
    "convA": [(64, 5, 2.69, 4, 2), (128, 6, 1.41, 6, 2)],
}
# a candidate the boundary cap turns down: in fp32 x and w_step are k/15 and
# 1/15, every partial is a multiple of 1/225, and adc_max 6.16 makes the step
# 22/225 -- one partial in 22 is an exact tie (24 % of the outputs flagged).
# adc_max 6.10 above is the same configuration off that lattice
REJECTED_CFG = ("linear", torch.float32, (128, 6, 6.16, 4, 2))
W_RANGE = (-0.5, 0.5)


def general_w(w_bits):
    """w_step, w_min of the B-bit grid the general weights sit on."""
    return dict(w_step=grid_step(w_bits, *W_RANGE), w_min=W_RANGE[0],
                w_bits=w_bits)


@lru_cache(maxsize=None)
def general_inputs(shape, dtype, w_bits, seed=1, batch=None):
    """fo.make_inputs with wq on the grid: fake_quant_forward over
    [-0.5, 0.5], rounded to the dtype (what a quantised layer hands the op)."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    if batch is not None:
        xs = (batch,) + xs[1:]
    inp = fo.make_inputs(xs, ws, dtype, seed)
    wq = ref_ops.fake_quant_forward(inp.wq.float(), w_bits, W_RANGE[0],
                                    W_RANGE[1], 0).to(dtype)
    return SimpleNamespace(x=inp.x, wq=wq, bias=inp.bias)


@lru_cache(maxsize=None)
def exact_inputs(shape, dtype, w_min=-8.0):
    """Integer inputs: x = randint(0,16), codes = randint(0,16) stored as
    wq = w_min + code (w_step 1), bias a multiple of 1/8. With a power-of-two
    ADC step every product, partial sum, v/step and the offset is exact in
    fp32 in any order."""
    kind, xs, ws, stride, pad = SHAPES[shape]
    gen = torch.Generator().manual_seed(23)
    x = torch.randint(0, 16, xs, generator=gen).float()
    code = torch.randint(0, 16, ws, generator=gen).float()
    bias = torch.randint(-8, 9, (ws[0],), generator=gen).float() / 8
    return SimpleNamespace(x=x.to(dtype), code=code.to(dtype),
                           wq=(code + w_min).to(dtype), bias=bias.to(dtype))


@lru_cache(maxsize=None)
def oracle(shape, dtype, inputs, mode, rows, bits, amax, w_bits, cell_bits,
           bias=True, batch=None):
    kind, xs, ws, stride, pad = SHAPES[shape]
    if inputs == "exact":
        inp, w = exact_inputs(shape, dtype), EXACT_W
        assert w_bits == w["w_bits"]
    else:
        inp = general_inputs(shape, dtype, w_bits, batch=batch)
        w = general_w(w_bits)
    b = inp.bias if bias else None
    if kind == "conv":
        return conv_blocked(inp.x, inp.wq, b, stride, pad, mode, rows, bits,
                            amax, w["w_step"], w["w_min"], w_bits, cell_bits)
    return linear_blocked(inp.x, inp.wq, b, mode, rows, bits, amax,
                          w["w_step"], w["w_min"], w_bits, cell_bits)


def tie_share(ref):
    return sum(float(((t - torch.floor(t)) == 0.5).double().mean())
               for t in ref.t) / len(ref.t)


def clip_share(ref):
    return ref.clipped / float(ref.n_partials)
