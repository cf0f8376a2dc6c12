"""fp64 oracle of the bit-sliced crossbar ops on PROGRAMMED cells
(ops.xbar_program_cells + ops.xbar_noisy_conv2d / _linear with ``cells=``).

The oracle takes the conductances G[T, K, n] as DATA (digit units, whatever
the kernel or the CPU twin wrote) and evaluates the bit-sliced model of
xbar_cells_oracle with G_t in place of the digit d_t:

    p_bt = w_step * sum_{k in b} x_k * G_t,k
    s_bt = max(p_bt, 0)                                                (abs)
         = max(w_step^2 * sum x * round_to_dtype(f32(G_t)^2) + p_bt, 0) (abs2)
    q_bt = step * clamp(rint(p_bt / step), 0, Qu)
    out  = sum_b (sum_t 2^(tE) q_bt + w_min * X_b) + bias

in fp64, with the fields xco.adc_report and xco.noise_variance read, so their
bounds are reused with A_bt = p_bt for |x|. The squares are rounded once to
the dtype of G, as the op stores them.

It also holds a numpy Philox4x32-10 with the key and counter layout of
csrc/common.h, which predicts the stuck-at uniform u of every cell, and the
configurations shared by test_xbar_programmed_oracle.py (CPU) and
test_xbar_programmed_gpu.py.
"""

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

import fused_noise_oracle as fo
import xbar_cells_oracle as xco
import xbar_oracle as xo
from noisynet_amd.ops import reference as ref_ops

SHAPES = xco.SHAPES

# the cell model of the fused-against-oracle tests
SIGMA, P_OFF, P_ON = 0.1, 0.02, 0.01
CHIP_SEED = 20240


def n_slices(w_bits, cell_bits):
    return -(-int(w_bits) // int(cell_bits))


def blocked(xm, G, bias, mode, xbar_rows, adc_bits, adc_max, w_step, w_min,
            cell_bits):
    """xco.blocked with the conductances G [T, K, n] as data. Returns the
    same fields (code / w_grid excepted)."""
    E, T = int(cell_bits), G.shape[0]
    ws, _, wm = xco.cell_params(w_step, w_min)
    Gd = G.detach().cpu()
    G64 = Gd.double()
    G2 = (Gd.float() * Gd.float()).to(Gd.dtype).double()   # rounded once
    xm = xm.double()
    n = xm.shape[1]
    assert G.shape[2] == n
    adc = adc_bits > 0
    step, qu = xco.adc_step(adc_bits, adc_max) if adc else (1.0, float("inf"))
    out = torch.zeros(xm.shape[0], G.shape[1], dtype=torch.float64)
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
            gt = G64[t][:, k0:k1]
            p = ws * (xb @ gt.t())
            tt = p / step
            if adc:
                r = torch.round(tt)
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
            As.append(ws * (xb.abs() @ gt.t()))
            if mode is not None:
                s = p
                if mode == "abs2":
                    s = ws * ws * (xb @ G2[t][:, k0:k1].t()) + p
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
        clipped=clipped, absmax=absmax,
        n_partials=T * nblocks * out.numel(),
        bias_abs=(torch.zeros(G.shape[1], dtype=torch.float64)
                  if bias is None else bias.double().abs()))


def rows_of(shape, x):
    kind, xs, ws, stride, pad = SHAPES[shape]
    if kind == "conv":
        return xo.conv_rows(x, ws[2], ws[3], stride, pad)
    return x.double()


def oracle(shape, inp, G, mode, rows, bits, amax, w_step, w_min, cell_bits,
           bias=True):
    return blocked(rows_of(shape, inp.x), G, inp.bias if bias else None, mode,
                   rows, bits, amax, w_step, w_min, cell_bits)


def folded_variance(shape, inp, G, rows, w_step, w_min, cell_bits):
    """The noise variance / factor a kernel would produce that wrongly took
    G for its own square (the one-bit ``fold_squares`` shortcut of the digit
    kernel): s = w_step^2 * sum x*G + p."""
    ref = oracle(shape, inp, G, "abs", rows, 0, 0.0, w_step, w_min, cell_bits)
    ws = ref.w_step
    return sum(sh * sh * (ws * p + p).clamp_min(0)
               for sh, p in zip(ref.shift, ref.s))


def digits(wq, w_step, w_min, w_bits, cell_bits):
    """[T, K, n] int64 digits of a weight tensor, rows in (r, s, c) order."""
    code = xco.codes(xo.weight_rows(wq), w_step, w_min, w_bits)
    E = int(cell_bits)
    return torch.stack([(code >> (t * E)) & (2 ** E - 1)
                        for t in range(n_slices(w_bits, E))])


def twin_cells(wq, w_bits, cell_bits, w_step, w_min, sigma, p_off, p_on,
               gen_seed):
    """G of the reference twin (CPU, torch.Generator stream)."""
    cell = ref_ops.xbar_cell_params(w_step, w_min, wq.device)
    gen = torch.Generator().manual_seed(gen_seed)
    return ref_ops.xbar_program_cells(wq, w_bits, cell_bits, cell, sigma,
                                      p_off, p_on, gen)


# ---------------------------------------------------------------------------
# Philox4x32-10 as csrc/common.h runs it: key = (seed lo, seed hi), counter =
# (ctr lo, ctr hi, 0, 0); ten rounds, the key bumped after each
# ---------------------------------------------------------------------------


def philox4x32(seed, counter):
    """Four uint32 words per counter (numpy uint64 array)."""
    counter = np.asarray(counter, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = counter & m32, counter >> np.uint64(32)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0          # < 2^64: exact in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & m32
        hi1, lo1 = p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = (hi1 ^ c1 ^ np.uint64(k0), lo1,
                          hi0 ^ c3 ^ np.uint64(k1), lo0)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def cell_uniforms(seed, T, K, n):
    """u of every cell [T, K, n]: u01(word 0) of the draw at counter
    (t*K + k)*n + i, in fp32 as the kernel computes it."""
    t, k, i = np.meshgrid(np.arange(T, dtype=np.uint64),
                          np.arange(K, dtype=np.uint64),
                          np.arange(n, dtype=np.uint64), indexing="ij")
    w0 = philox4x32(seed, (t * np.uint64(K) + k) * np.uint64(n) + i)[0]
    u = w0.astype(np.float32) * np.float32(1.0 / 4294967296.0)
    return torch.from_numpy(u)


def predict_stuck(dig, seed, p_off, p_on, cell_bits):
    """G at sigma = 0: 0 where u < p_off, 2^E - 1 where u < p_off + p_on,
    else the digit (the thresholds in fp32, as the kernel compares)."""
    T, K, n = dig.shape
    u = cell_uniforms(seed, T, K, n)
    po = np.float32(p_off)
    pa = np.float32(po + np.float32(p_on))
    top = float(2 ** int(cell_bits) - 1)
    d = dig.double()
    return torch.where(u < float(po), torch.zeros_like(d),
                       torch.where(u < float(pa), torch.full_like(d, top), d))


# ---------------------------------------------------------------------------
# fused against the oracle, noise off, ADC on: (rows, adc_bits, adc_max,
# w_bits, cell_bits) as in xco.GENERAL_CFGS, each adc_max chosen on the CPU
# with the reference twin's G at GEN_SEEDS (test_xbar_programmed_oracle.py
# asserts the caps): at most 0.02 of the outputs flagged there, the clip
# share inside (0, 0.5)
# ---------------------------------------------------------------------------

GEN_SEEDS = (11, 12, 13)
# (rows, adc_bits, w_bits, cell_bits) are those of xco.GENERAL_CFGS; two
# ranges of the linear shape are wider than there (0.30 and 13.4 clip three
# partials in four on these cells)
PROG_CFGS = {
    "linear": [(64, 5, 1.10, 4, 1), (128, 6, 6.10, 4, 2), (32, 4, 0.52, 6, 2),
               (64, 5, 17.3, 4, 4)],
    "convA": [(64, 5, 2.69, 4, 2), (128, 6, 1.41, 6, 2)],
}
assert all([(c[0], c[1], c[3], c[4]) for c in PROG_CFGS[s]]
           == [(c[0], c[1], c[3], c[4]) for c in xco.GENERAL_CFGS[s]]
           for s in PROG_CFGS)
# the candidate of xco.REJECTED_CFG sits on the same lattice whatever the
# cells hold at sigma = 0; with sigma = 0.1 the conductances leave the lattice
# and the tie-heavy step is harmless, so the rejected candidate here is one
# whose range is too small: nearly every partial clips
REJECTED_CFG = ("linear", torch.float32, (128, 6, 0.61, 4, 2))


@lru_cache(maxsize=None)
def twin_oracle(shape, dtype, cfg, gen_seed, bias=True):
    rows, bits, amax, B, E = cfg
    inp = xco.general_inputs(shape, dtype, B)
    w = xco.general_w(B)
    G = twin_cells(inp.wq, B, E, w["w_step"], w["w_min"], SIGMA, P_OFF, P_ON,
                   gen_seed)
    return oracle(shape, inp, G, None, rows, bits, amax, w["w_step"],
                  w["w_min"], E, bias), G
