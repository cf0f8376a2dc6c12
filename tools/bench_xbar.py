#!/usr/bin/env python3
"""Time the fused tiled-crossbar op against its two neighbours on the GPU.

At the flagship's own shapes at batch 2048, bf16, noise 'abs2' + 6-bit ADC:

  conv2    x [2048, 65, 14, 14], w [120, 65, 5, 5]   (n = 1625 crossbar rows)
  linear1  [2048, 3000] x [390, 3000]

and for xbar_rows in {64, 128, 256}:

  (a) xbar      ops.xbar_noisy_conv2d / xbar_noisy_linear: one kernel, every
                block's noise and ADC in registers
  (b) unblocked ops.fused_noisy_conv2d / fused_noisy_linear: today's one
                unbounded crossbar (no ADC; recorded, not a gate)
  (c) eager     what a user would write without (a): im2col once, then per
                block slice -> two bf16 matmuls -> randn noise -> round /
                clamp -> add, every partial through memory
  (d) diff      (a) with differential=True: W+ / W- columns, two noise draws
                and two unipolar ADCs per block, still one kernel
  (c') eager_diff  the eager composition of the differential model: four
                bf16 matmuls per block, twice those of (c)
  (e) serial    (a) with bit-serial inputs: in_bits 4, dac_bits 1 (J = 4
                slices) and 2 (J = 2), J noise draws and J ADC conversions
                per block, still one kernel
  (c") eager_serial  the eager bit-serial composition: per block and slice two
                bf16 matmuls, randn noise, round / clamp and the shift-add,
                J x the matmuls of (c); the slice row matrices are built once,
                outside the timed region
  (f) cells     (a) with bit-sliced weights: w_bits 4, cell_bits 1 (T = 4
                slices) and 2 (T = 2), the weights put on the 4-bit grid
                beforehand; T noise draws and T unipolar ADC conversions per
                block plus the digital offset w_min * sum x, still one kernel
  (f') eager_cells  the eager bit-sliced composition: per block and slice two
                bf16 matmuls (digits and their squares), randn noise, round /
                clamp and the shift-add, per block the offset; the digit
                matrices are built once, outside the timed region
  (g) prog      (f) on programmed cells: ops.xbar_program_cells writes the
                conductances G once (sigma 0.1, 1 % stuck off, 0.5 % stuck
                on) and the fused op reads the T slices of G in place of the
                digits; no one-bit shortcut for the squares. 'program' is
                the programming kernel on its own
  (f") eager_prog  (f') given the same G: the slices of G and their squares
                as the digit matrices. The condition is (g) + program <
                (f") at every row count

Device events around windows of at least --window seconds after a warm-up,
the variants alternating over --rounds rounds in one process; the median
round is reported. Prints one JSON line per (layer, xbar_rows). There is no
CPU fallback: a time is a GPU time or it is not reported.

--resource-usage needs no GPU: it compiles csrc/xbar_fwd.hip,
csrc/xbar_serial.hip and csrc/xbar_cells.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage and prints VGPRs, LDS and scratch of
every xbar_fwd_kernel, xbar_diff_fwd_kernel, xbar_serial_fwd_kernel and
xbar_cells_fwd_kernel instantiation (the programmed-cell ones, PROG, listed
apart) and of xbar_program_cells_kernel.
"""

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from noisynet_amd import ops  # noqa: E402
from noisynet_amd.ops import reference as ref  # noqa: E402

XBAR_SOURCES = ('xbar_fwd.hip', 'xbar_serial.hip', 'xbar_cells.hip')

LAYERS = {
    'conv2': dict(kind='conv', x=(2048, 65, 14, 14), w=(120, 65, 5, 5)),
    'linear1': dict(kind='linear', x=(2048, 3000), w=(390, 3000)),
}
MODE, FACTOR, ADC_BITS, ADC_MAX = 'abs2', 0.05, 6, 3.0
# bit-serial inputs: the activations are on the 4-bit grid k/15
IN_BITS, X_STEP, DAC_BITS = 4, 1.0 / 15.0, (1, 2)
# a slice partial is far smaller than a full-code one: +-3 would round nearly
# all of them to 0 and make the agreement check empty
SERIAL_ADC_MAX = 0.25
# bit-sliced weights: the 4-bit grid over [-0.3, 0.3] (3 sigma of the weights)
W_BITS, W_RANGE, CELL_BITS = 4, (-0.3, 0.3), (1, 2)
W_STEP = (W_RANGE[1] - W_RANGE[0]) / (2 ** W_BITS - 1)
# the range [0, adc_max] of one unipolar slice conversion
CELL_ADC_MAX = 4.0
# programmed cells: conductance variation and stuck-at rates of the chip
CELL_VAR, CELL_P_OFF, CELL_P_ON = 0.1, 0.01, 0.005


def eager_blocked(xm, wq, fw, factor, xbar_rows, step, inv_step, qm,
                  fp32_matmul=False):
    """Per-block composition of stock torch ops on row matrices (bf16
    matmuls, fp32 epilogue; fp32 matmuls for the agreement check, where a
    partial rounded to bf16 would land on another ADC level)."""
    if fp32_matmul:
        xm, wq, fw = xm.float(), wq.float(), fw.float()
    n = xm.shape[1]
    out = None
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        p = (xb @ wq[:, k0:k1].t()).float()
        s = (xb @ fw[:, k0:k1].t()).float().clamp_min(0)
        v = p + torch.randn_like(p) * (factor * s).sqrt()
        q = step * torch.round(v * inv_step).clamp(-qm, qm)
        out = q if out is None else out + q
    return out


def eager_diff(xm, wq, wr, factor, xbar_rows, step, inv_step, qu, mode=MODE,
               fp32_matmul=False):
    """The differential model composed of stock torch ops: per block and per
    column a wq+- matmul, an f+- matmul, randn noise and a unipolar round /
    clamp; the two columns subtracted, every partial through memory. The
    split weight matrices are prepared once, outside the timed region."""
    wqs, fws = wq, wr       # tuples (positive column, negative column)
    if fp32_matmul:
        xm = xm.float()
        wqs = tuple(w.float() for w in wqs)
        fws = tuple(w.float() for w in fws)
    n = xm.shape[1]
    out = None
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        qs = []
        for col in range(2):
            p = (xb @ wqs[col][:, k0:k1].t()).float()
            s = (xb @ fws[col][:, k0:k1].t()).float().clamp_min(0)
            v = p + torch.randn_like(p) * (factor * s).sqrt()
            qs.append(step * torch.round(v * inv_step).clamp(0, qu))
        q = qs[0] - qs[1]
        out = q if out is None else out + q
    return out


def eager_serial(slices, wq, fw, factor, xbar_rows, step, inv_step, qm,
                 x_step, dac_bits, fp32_matmul=False):
    """The bit-serial model composed of stock torch ops: per block and per
    slice a wq matmul, an f matmul, randn noise and a round / clamp, then the
    shift-add; every partial through memory. ``slices`` are the row matrices
    d_j, prepared once, outside the timed region."""
    if fp32_matmul:
        slices = [d.float() for d in slices]
        wq, fw = wq.float(), fw.float()
    n = wq.shape[1]
    out = None
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        for j, d in enumerate(slices):
            xb = d[:, k0:k1]
            p = x_step * (xb @ wq[:, k0:k1].t()).float()
            s = (x_step * (xb @ fw[:, k0:k1].t()).float()).clamp_min(0)
            v = p + torch.randn_like(p) * (factor * s).sqrt()
            q = float(2 ** (j * dac_bits)) \
                * (step * torch.round(v * inv_step).clamp(-qm, qm))
            out = q if out is None else out + q
    return out


def eager_cells(xm, digits, squares, factor, xbar_rows, step, inv_step, qu,
                w_step, w_min, cell_bits, fp32_matmul=False):
    """The bit-sliced-weight model composed of stock torch ops: per block and
    per slice a digit matmul, a squared-digit matmul, randn noise and a
    unipolar round / clamp, then the shift-add; per block the offset
    w_min * sum x; every partial through memory. ``digits`` / ``squares`` are
    the matrices d_t / d_t^2, prepared once, outside the timed region."""
    if fp32_matmul:
        xm = xm.float()
        digits = [d.float() for d in digits]
        squares = [d.float() for d in squares]
    n = xm.shape[1]
    out = None
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        for t, (d, d2) in enumerate(zip(digits, squares)):
            p = w_step * (xb @ d[:, k0:k1].t()).float()
            s = (w_step * w_step * (xb @ d2[:, k0:k1].t()).float()
                 + p).clamp_min(0)
            v = p + torch.randn_like(p) * (factor * s).sqrt()
            q = float(2 ** (t * cell_bits)) \
                * (step * torch.round(v * inv_step).clamp(0, qu))
            out = q if out is None else out + q
        out = out + w_min * xb.float().sum(dim=1, keepdim=True)
    return out


def make_digits(wq_rows, w_step, w_min, w_bits, cell_bits):
    cell = ref.xbar_cell_params(w_step, w_min, wq_rows.device)
    code = torch.round((wq_rows.float() - cell[2]) * cell[1]) \
        .clamp(0, 2 ** w_bits - 1).to(torch.int32)
    return [((code >> (t * cell_bits)) & (2 ** cell_bits - 1))
            .to(wq_rows.dtype).contiguous()
            for t in range(-(-w_bits // cell_bits))]


def make_slices(xm, x_step, in_bits, dac_bits):
    inv = 1.0 / torch.tensor(x_step, dtype=torch.float32)
    code = torch.round(xm.float() * inv.to(xm.device)) \
        .clamp(0, 2 ** in_bits - 1).to(torch.int32)
    return [((code >> (j * dac_bits)) & (2 ** dac_bits - 1)).to(xm.dtype)
            for j in range(-(-in_bits // dac_bits))]


def timed(fn, window, min_calls=3):
    """seconds per call over a window >= ``window``."""
    calls, total = 0, 0.0
    while total < window or calls < min_calls:
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        n = fn()
        stop.record()
        stop.synchronize()
        total += start.elapsed_time(stop) / 1e3
        calls += n
    return total / calls


def bench_layer(name, spec, rows_list, window, rounds, reps):
    dev, dtype = torch.device('cuda'), torch.bfloat16
    gen = torch.Generator().manual_seed(0)
    x = (torch.randint(0, 16, spec['x'], generator=gen).float() / 15).to(dtype)
    wq = (torch.randn(spec['w'], generator=gen) * 0.1).to(dtype)
    wr = (torch.randn(spec['w'], generator=gen) * 0.1).to(dtype)
    x, wq, wr = x.to(dev), wq.to(dev), wr.to(dev)
    conv = spec['kind'] == 'conv'
    if conv:
        x = x.contiguous(memory_format=torch.channels_last)
        wq = wq.contiguous(memory_format=torch.channels_last)
        wr = wr.contiguous(memory_format=torch.channels_last)
    factor = torch.tensor([FACTOR], device=dev)
    adc = ref.xbar_adc_params(ADC_BITS, ADC_MAX, dev)
    step, inv_step = adc[0], adc[1]
    qm = float(2 ** (ADC_BITS - 1) - 1)
    wq_rows = ref.xbar_weight_rows(wq).contiguous()
    aw = ref.xbar_weight_rows(wr).abs()
    fw_rows = (aw * aw + aw).contiguous()
    n = wq_rows.shape[1]
    # differential columns: unipolar step, split weight matrices
    adc_u = ref.xbar_adc_params(ADC_BITS, ADC_MAX, dev, unipolar=True)
    step_u, inv_step_u = adc_u[0], adc_u[1]
    qu = float(2 ** ADC_BITS - 1)
    wq_cols = (wq_rows.clamp_min(0).contiguous(),
               (-wq_rows).clamp_min(0).contiguous())
    wr_rows = ref.xbar_weight_rows(wr)
    zero = torch.zeros_like(fw_rows)
    fw_cols = (torch.where(wr_rows > 0, fw_rows, zero).contiguous(),
               torch.where(wr_rows < 0, fw_rows, zero).contiguous())

    def run_unblocked():
        for _ in range(reps):
            if conv:
                ops.fused_noisy_conv2d(x, wq, wr, None, 1, 0, MODE, factor)
            else:
                ops.fused_noisy_linear(x, wq, wr, None, MODE, factor)
        return reps

    results = []
    for rows in rows_list:
        def run_xbar():
            for _ in range(reps):
                if conv:
                    ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, MODE, factor,
                                          rows, ADC_BITS, ADC_MAX)
                else:
                    ops.xbar_noisy_linear(x, wq, wr, None, MODE, factor, rows,
                                          ADC_BITS, ADC_MAX)
            return reps

        def run_eager():
            xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
                if conv else x
            eager_blocked(xm, wq_rows, fw_rows, factor, rows, step, inv_step,
                          qm)
            return 1

        def run_diff():
            for _ in range(reps):
                if conv:
                    ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, MODE, factor,
                                          rows, ADC_BITS, ADC_MAX,
                                          differential=True)
                else:
                    ops.xbar_noisy_linear(x, wq, wr, None, MODE, factor, rows,
                                          ADC_BITS, ADC_MAX,
                                          differential=True)
            return reps

        def run_eager_diff():
            xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
                if conv else x
            eager_diff(xm, wq_cols, fw_cols, factor, rows, step_u, inv_step_u,
                       qu)
            return 1

        variants = {'xbar': run_xbar, 'unblocked': run_unblocked,
                    'eager': run_eager, 'diff': run_diff,
                    'eager_diff': run_eager_diff}
        dac = ref.xbar_dac_params(X_STEP, dev)
        adc_s = ref.xbar_adc_params(ADC_BITS, SERIAL_ADC_MAX, dev)
        step_s, inv_step_s = adc_s[0], adc_s[1]
        xm_all = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
            if conv else x
        slices, moved_serial = {}, {}
        for D in DAC_BITS:
            slices[D] = make_slices(xm_all, X_STEP, IN_BITS, D)

            def run_serial(D=D):
                kw = dict(in_bits=IN_BITS, dac_bits=D, x_step=X_STEP)
                for _ in range(reps):
                    if conv:
                        ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, MODE,
                                              factor, rows, ADC_BITS,
                                              SERIAL_ADC_MAX, **kw)
                    else:
                        ops.xbar_noisy_linear(x, wq, wr, None, MODE, factor,
                                              rows, ADC_BITS, SERIAL_ADC_MAX,
                                              **kw)
                return reps

            def run_eager_serial(D=D):
                eager_serial(slices[D], wq_rows, fw_rows, factor, rows,
                             step_s, inv_step_s, qm, dac[0], D)
                return 1

            variants['serial_d%d' % D] = run_serial
            variants['eager_serial_d%d' % D] = run_eager_serial
        del xm_all
        # bit-sliced weights: wq on the grid, digit matrices per cell width
        wg = ref.fake_quant_forward(wq.float(), W_BITS, W_RANGE[0],
                                    W_RANGE[1], 0).to(dtype)
        if conv:
            wg = wg.contiguous(memory_format=torch.channels_last)
        wg_rows = ref.xbar_weight_rows(wg).contiguous()
        cell = ref.xbar_cell_params(W_STEP, W_RANGE[0], dev)
        adc_c = ref.xbar_adc_params(ADC_BITS, CELL_ADC_MAX, dev, unipolar=True)
        step_c, inv_step_c = adc_c[0], adc_c[1]
        ckw = dict(w_bits=W_BITS, w_step=W_STEP, w_min=W_RANGE[0])
        digits, squares, moved_cells = {}, {}, {}
        chips, chip_rows, chip_squares, moved_prog = {}, {}, {}, {}
        for E in CELL_BITS:
            digits[E] = make_digits(wg_rows, W_STEP, W_RANGE[0], W_BITS, E)
            squares[E] = [(d * d).contiguous() for d in digits[E]]

            def run_cells(E=E):
                for _ in range(reps):
                    if conv:
                        ops.xbar_noisy_conv2d(x, wg, wg, None, 1, 0, MODE,
                                              factor, rows, ADC_BITS,
                                              CELL_ADC_MAX, cell_bits=E, **ckw)
                    else:
                        ops.xbar_noisy_linear(x, wg, wg, None, MODE, factor,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, **ckw)
                return reps

            def run_eager_cells(E=E):
                xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
                    if conv else x
                eager_cells(xm, digits[E], squares[E], factor, rows, step_c,
                            inv_step_c, qu, cell[0], cell[2], E)
                return 1

            variants['cells_e%d' % E] = run_cells
            variants['eager_cells_e%d' % E] = run_eager_cells
            # the same on programmed cells
            pkw = dict(sigma=CELL_VAR, p_stuck_off=CELL_P_OFF,
                       p_stuck_on=CELL_P_ON, seed=1)
            chips[E] = ops.xbar_program_cells(wg, W_BITS, E, W_STEP,
                                              W_RANGE[0], **pkw)
            chip_rows[E] = [g.contiguous() for g in chips[E]]
            chip_squares[E] = [(g.float() * g.float()).to(dtype)
                               for g in chip_rows[E]]

            def run_prog(E=E):
                for _ in range(reps):
                    if conv:
                        ops.xbar_noisy_conv2d(x, wg, wg, None, 1, 0, MODE,
                                              factor, rows, ADC_BITS,
                                              CELL_ADC_MAX, cell_bits=E,
                                              cells=chips[E], **ckw)
                    else:
                        ops.xbar_noisy_linear(x, wg, wg, None, MODE, factor,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, cells=chips[E],
                                              **ckw)
                return reps

            def run_program(E=E):
                for _ in range(reps):
                    ops.xbar_program_cells(wg, W_BITS, E, W_STEP, W_RANGE[0],
                                           **pkw)
                return reps

            def run_eager_prog(E=E):
                xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
                    if conv else x
                eager_cells(xm, chip_rows[E], chip_squares[E], factor, rows,
                            step_c, inv_step_c, qu, cell[0], cell[2], E)
                return 1

            variants['prog_e%d' % E] = run_prog
            variants['program_e%d' % E] = run_program
            variants['eager_prog_e%d' % E] = run_eager_prog
        with torch.no_grad():
            # results must agree before speeds are compared: noise off, the
            # fused op against the eager composition on the same blocks
            if conv:
                a = ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, None, 0.0,
                                          rows, ADC_BITS, ADC_MAX)
                a = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])
                xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0)
            else:
                a = ops.xbar_noisy_linear(x, wq, wr, None, None, 0.0, rows,
                                          ADC_BITS, ADC_MAX)
                xm = x
            e = eager_blocked(xm, wq_rows, fw_rows,
                              torch.zeros(1, device=dev), rows, step,
                              inv_step, qm, fp32_matmul=True)
            diff = (a.float() - e.float()).abs()
            moved = float((diff > 0.5 * float(step)).float().mean())
            # the same check for the differential op
            if conv:
                a = ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, None, 0.0,
                                          rows, ADC_BITS, ADC_MAX,
                                          differential=True)
                a = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])
            else:
                a = ops.xbar_noisy_linear(x, wq, wr, None, None, 0.0, rows,
                                          ADC_BITS, ADC_MAX,
                                          differential=True)
            e = eager_diff(xm, wq_cols, fw_cols, torch.zeros(1, device=dev),
                           rows, step_u, inv_step_u, qu, fp32_matmul=True)
            del xm
            # the unipolar step is half the bipolar one, below the bf16
            # spacing of the largest outputs: round the reference alike
            diff = (a.float() - e.to(a.dtype).float()).abs()
            moved_diff = float((diff > 0.5 * float(step_u)).float().mean())
            # and for the bit-serial op: outputs off by more than half a step
            for D in DAC_BITS:
                kw = dict(in_bits=IN_BITS, dac_bits=D, x_step=X_STEP)
                if conv:
                    a = ops.xbar_noisy_conv2d(x, wq, wr, None, 1, 0, None,
                                              0.0, rows, ADC_BITS,
                                              SERIAL_ADC_MAX, **kw)
                    a = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])
                else:
                    a = ops.xbar_noisy_linear(x, wq, wr, None, None, 0.0,
                                              rows, ADC_BITS, SERIAL_ADC_MAX,
                                              **kw)
                e = eager_serial(slices[D], wq_rows, fw_rows,
                                 torch.zeros(1, device=dev), rows, step_s,
                                 inv_step_s, qm, dac[0], D, fp32_matmul=True)
                diff = (a.float() - e.to(a.dtype).float()).abs()
                moved_serial[D] = float(
                    (diff > 0.5 * float(step_s)).float().mean())
            # and for the bit-sliced weights (unipolar slices plus the offset)
            xm = ref.xbar_conv_rows(x, spec['w'][2], spec['w'][3], 1, 0) \
                if conv else x
            for E in CELL_BITS:
                if conv:
                    a = ops.xbar_noisy_conv2d(x, wg, wg, None, 1, 0, None, 0.0,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, **ckw)
                    a = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])
                else:
                    a = ops.xbar_noisy_linear(x, wg, wg, None, None, 0.0,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, **ckw)
                e = eager_cells(xm, digits[E], squares[E],
                                torch.zeros(1, device=dev), rows, step_c,
                                inv_step_c, qu, cell[0], cell[2], E,
                                fp32_matmul=True)
                diff = (a.float() - e.to(a.dtype).float()).abs()
                moved_cells[E] = float(
                    (diff > 0.5 * float(step_c)).float().mean())
                if conv:
                    a = ops.xbar_noisy_conv2d(x, wg, wg, None, 1, 0, None, 0.0,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, cells=chips[E],
                                              **ckw)
                    a = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])
                else:
                    a = ops.xbar_noisy_linear(x, wg, wg, None, None, 0.0,
                                              rows, ADC_BITS, CELL_ADC_MAX,
                                              cell_bits=E, cells=chips[E],
                                              **ckw)
                e = eager_cells(xm, chip_rows[E], chip_squares[E],
                                torch.zeros(1, device=dev), rows, step_c,
                                inv_step_c, qu, cell[0], cell[2], E,
                                fp32_matmul=True)
                diff = (a.float() - e.to(a.dtype).float()).abs()
                moved_prog[E] = float(
                    (diff > 0.5 * float(step_c)).float().mean())
            del xm
            for fn in variants.values():    # warm-up: code objects, allocator
                fn()
            torch.cuda.synchronize()
            rr = {k: [] for k in variants}
            for _ in range(rounds):         # alternate the variants
                for k, fn in variants.items():
                    rr[k].append(timed(fn, window))
        sec = {k: statistics.median(v) for k, v in rr.items()}
        res = {
            'bench': 'xbar_adc', 'device': torch.cuda.get_device_name(0),
            'layer': name, 'x': list(spec['x']), 'w': list(spec['w']),
            'crossbar_rows_total': n, 'xbar_rows': rows,
            'blocks': -(-n // rows), 'dtype': 'bf16', 'sigma_mode': MODE,
            'adc_bits': ADC_BITS, 'adc_max': ADC_MAX, 'window_s': window,
            'rounds': rounds,
            'xbar_ms': round(sec['xbar'] * 1e3, 4),
            'unblocked_ms': round(sec['unblocked'] * 1e3, 4),
            'eager_ms': round(sec['eager'] * 1e3, 4),
            'xbar_over_unblocked': round(sec['xbar'] / sec['unblocked'], 3),
            'eager_over_xbar': round(sec['eager'] / sec['xbar'], 2),
            'diff_ms': round(sec['diff'] * 1e3, 4),
            'eager_diff_ms': round(sec['eager_diff'] * 1e3, 4),
            'diff_over_xbar': round(sec['diff'] / sec['xbar'], 3),
            'eager_diff_over_diff': round(sec['eager_diff'] / sec['diff'], 2),
            'rounds_ms': {k: [round(t * 1e3, 4) for t in v]
                          for k, v in rr.items()},
            'noise_off_outputs_off_by_a_step_vs_eager': moved,
            'diff_noise_off_outputs_off_by_a_step_vs_eager': moved_diff,
            'in_bits': IN_BITS, 'serial_adc_max': SERIAL_ADC_MAX,
        }
        for D in DAC_BITS:
            ser, eag = sec['serial_d%d' % D], sec['eager_serial_d%d' % D]
            res['serial_d%d_ms' % D] = round(ser * 1e3, 4)
            res['eager_serial_d%d_ms' % D] = round(eag * 1e3, 4)
            res['serial_d%d_over_xbar' % D] = round(ser / sec['xbar'], 3)
            res['eager_serial_d%d_over_serial' % D] = round(eag / ser, 2)
            res['serial_d%d_noise_off_outputs_off_by_a_step_vs_eager' % D] = \
                moved_serial[D]
        res.update(w_bits=W_BITS, cell_adc_max=CELL_ADC_MAX)
        for E in CELL_BITS:
            cel, eag = sec['cells_e%d' % E], sec['eager_cells_e%d' % E]
            res['cells_e%d_ms' % E] = round(cel * 1e3, 4)
            res['eager_cells_e%d_ms' % E] = round(eag * 1e3, 4)
            res['cells_e%d_over_xbar' % E] = round(cel / sec['xbar'], 3)
            res['eager_cells_e%d_over_cells' % E] = round(eag / cel, 2)
            res['cells_e%d_noise_off_outputs_off_by_a_step_vs_eager' % E] = \
                moved_cells[E]
        res.update(cell_var=CELL_VAR, cell_stuck_off=CELL_P_OFF,
                   cell_stuck_on=CELL_P_ON)
        for E in CELL_BITS:
            prg, one = sec['prog_e%d' % E], sec['program_e%d' % E]
            eag = sec['eager_prog_e%d' % E]
            res['prog_e%d_ms' % E] = round(prg * 1e3, 4)
            res['program_e%d_ms' % E] = round(one * 1e3, 4)
            res['eager_prog_e%d_ms' % E] = round(eag * 1e3, 4)
            res['prog_e%d_over_cells' % E] = round(
                prg / sec['cells_e%d' % E], 3)
            res['eager_prog_e%d_over_prog_plus_program' % E] = round(
                eag / (prg + one), 2)
            res['prog_e%d_noise_off_outputs_off_by_a_step_vs_eager' % E] = \
                moved_prog[E]
        del slices, digits, squares, chips, chip_rows, chip_squares
        print(json.dumps(res), flush=True)
        results.append(res)
    return results


def resource_usage():
    """VGPRs / LDS / scratch of every xbar_fwd_kernel and
    xbar_diff_fwd_kernel instantiation, from the compiler's own remarks
    (device-only compile for gfx950, no GPU needed)."""
    from torch.utils import cpp_extension as ce
    import sysconfig
    inc = ['-I' + p for p in ce.include_paths(device_type='cuda')]
    inc.append('-I' + sysconfig.get_paths()['include'])
    # side by side (each takes minutes); the remarks go to files, since a
    # pipe that nobody reads yet would stall its compiler once it is full
    procs = []
    for name in XBAR_SOURCES:
        cmd = ['hipcc', '-c', os.path.join(REPO, 'csrc', name), '-o',
               os.devnull, '-O3', '-std=c++17',
               '--offload-arch=gfx950', '--offload-device-only',
               '-D__HIP_PLATFORM_AMD__=1', '-DUSE_ROCM=1', '-DTORCH_HIP=1',
               '-DTORCH_EXTENSION_NAME=noisynet_hip', '-fno-gpu-rdc',
               '-mllvm', '--amdgpu-mfma-vgpr-form', '-x', 'hip',
               '-Rpass-analysis=kernel-resource-usage'] + inc
        err = tempfile.TemporaryFile(mode='w+')
        procs.append((cmd, subprocess.Popen(cmd, stderr=err), err))
    text = ''
    for cmd, p, err in procs:
        rc = p.wait()
        err.seek(0)
        text += err.read()
        err.close()
        if rc != 0:
            raise subprocess.CalledProcessError(rc, cmd)
    return parse_resource_usage(text)


def parse_resource_usage(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = {'kernel': m.group(1)} \
                if ('xbar_fwd_kernel' in m.group(1)
                    or 'xbar_diff_fwd_kernel' in m.group(1)
                    or 'xbar_serial_fwd_kernel' in m.group(1)
                    or 'xbar_cells_fwd_kernel' in m.group(1)
                    or 'xbar_program_cells_kernel' in m.group(1)) else None
            if cur is not None:
                rows.append(cur)
            continue
        if cur is None:
            continue
        m = re.search(r'remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize '
                      r'\[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|'
                      r'VGPRs Spill|LDS Size \[bytes/block\]): (\d+)', line)
        if m:
            cur[m.group(1)] = int(m.group(2))
    for r in rows:
        print(json.dumps(r))
    # the dynamic LDS tiles are sized at launch: (64 + 3*64) rows of 80 B
    # (16-bit) or 144 B (fp32), (64 + 5*64) rows on differential columns, on
    # top of the static bytes reported above
    diff = [r for r in rows if 'xbar_diff_fwd_kernel' in r['kernel']]
    serial = [r for r in rows if 'xbar_serial_fwd_kernel' in r['kernel']]
    # the trailing template flag PROG (programmed cells) is the fourth ELb
    all_cells = [r for r in rows if 'xbar_cells_fwd_kernel' in r['kernel']]
    cells = [r for r in all_cells if r['kernel'].split('ELb')[3][0] == '0']
    prog = [r for r in all_cells if r['kernel'].split('ELb')[3][0] == '1']
    program = [r for r in rows if 'xbar_program_cells_kernel' in r['kernel']]
    summarise('xbar_fwd_kernel',
              [r for r in rows if r not in diff and r not in serial
               and r not in all_cells and r not in program], 256)
    summarise('xbar_diff_fwd_kernel', diff, 384)
    # (J*64 + 3*64) rows; the mangled name carries T (DF16b / DF16_ / f), J,
    # SIGMA_MODE, ADC and TELEM as I<T>Li<J>ELi<mode>ELb<adc>ELb<telem>E
    for J in (1, 2, 3, 4):
        of_j = [r for r in serial
                if re.search(r'kernelI\w+?Li%dELi\dELb' % J, r['kernel'])]
        summarise('xbar_serial_fwd_kernel J=%d' % J, of_j, 64 * J + 192)
        steady = [r for r in of_j if r['kernel'].split('ELb')[2][0] == '0'
                  and 'kernelIf' not in r['kernel']]
        summarise('xbar_serial_fwd_kernel J=%d, 16-bit, no telemetry' % J,
                  steady, 64 * J + 192)
    # (64 + T*64) rows, twice the T*64 with abs2 (the tiles of squares)
    for T in (1, 2, 3, 4):
        of_t = [r for r in cells
                if re.search(r'kernelI\w+?Li%dELi\dELb' % T, r['kernel'])]
        summarise('xbar_cells_fwd_kernel T=%d' % T, of_t, 64 + 128 * T)
        steady = [r for r in of_t if r['kernel'].split('ELb')[2][0] == '0'
                  and 'kernelIf' not in r['kernel']]
        summarise('xbar_cells_fwd_kernel T=%d, 16-bit, no telemetry' % T,
                  steady, 64 + 128 * T)
    # programmed cells: the same tiles, read from G instead of derived
    for T in (1, 2, 3, 4):
        of_t = [r for r in prog
                if re.search(r'kernelI\w+?Li%dELi\dELb' % T, r['kernel'])]
        summarise('xbar_cells_fwd_kernel PROG T=%d' % T, of_t, 64 + 128 * T)
        steady = [r for r in of_t if r['kernel'].split('ELb')[2][0] == '0'
                  and 'kernelIf' not in r['kernel']]
        summarise('xbar_cells_fwd_kernel PROG T=%d, 16-bit, no telemetry' % T,
                  steady, 64 + 128 * T)
    summarise('xbar_program_cells_kernel', program, 0)
    return rows


def summarise(label, rows, lds_rows):
    print(json.dumps({
        'summary': label,
        'kernels': len(rows),
        'max_VGPRs': max(r['VGPRs'] for r in rows),
        'max_AGPRs': max(r['AGPRs'] for r in rows),
        'max_scratch_bytes_per_lane':
            max(r['ScratchSize [bytes/lane]'] for r in rows),
        'max_VGPR_spill': max(r['VGPRs Spill'] for r in rows),
        'min_occupancy_waves_per_simd':
            min(r['Occupancy [waves/SIMD]'] for r in rows),
        'max_static_LDS_bytes': max(r['LDS Size [bytes/block]'] for r in rows),
        'dynamic_LDS_bytes': {'bf16/fp16': lds_rows * 80,
                              'fp32': lds_rows * 144}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows', type=int, nargs='+', default=[64, 128, 256])
    ap.add_argument('--layers', nargs='+', default=list(LAYERS),
                    choices=list(LAYERS))
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10,
                    help='fused calls per timed event pair')
    ap.add_argument('--resource-usage', action='store_true')
    args = ap.parse_args()
    if args.resource_usage:
        resource_usage()
        return
    if not torch.cuda.is_available():
        raise SystemExit('bench_xbar needs a GPU: nothing measured')
    slower = []
    for name in args.layers:
        for r in bench_layer(name, LAYERS[name], args.rows, args.window,
                             args.rounds, args.reps):
            if not r['xbar_ms'] < r['eager_ms']:
                slower.append((name, r['xbar_rows']))
            if not r['diff_ms'] < r['eager_diff_ms']:
                slower.append((name, r['xbar_rows'], 'differential'))
            for D in DAC_BITS:
                if not r['serial_d%d_ms' % D] < r['eager_serial_d%d_ms' % D]:
                    slower.append((name, r['xbar_rows'],
                                   'bit-serial dac_bits %d' % D))
            for E in CELL_BITS:
                if not r['cells_e%d_ms' % E] < r['eager_cells_e%d_ms' % E]:
                    slower.append((name, r['xbar_rows'],
                                   'bit-sliced cell_bits %d' % E))
                if not (r['prog_e%d_ms' % E] + r['program_e%d_ms' % E]
                        < r['eager_prog_e%d_ms' % E]):
                    slower.append((name, r['xbar_rows'],
                                   'programmed cells cell_bits %d' % E))
    if slower:
        raise SystemExit('fused op not faster than the eager composition at '
                         '%s' % slower)


if __name__ == '__main__':
    main()
