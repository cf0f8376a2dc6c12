"""The 4-layer CIFAR-10 ConvNet ("NoisyNet" proper).

Architecture and forward semantics reproduce reference noisynet.py:326-695:
conv1(3->fm1*w, fs x fs) -> [noise] -> maxpool2x2 -> bn1 -> relu -> clip ->
[dropout_conv] -> [quant] -> conv2 -> [noise] -> pool -> bn2 -> relu -> clip
-> [dropout] -> flatten -> [quant] -> linear1 -> [noise] -> bn3 -> relu ->
clip -> [dropout] -> [quant] -> linear2 -> [noise] -> bn4.

MI355X-first execution: when no introspection flag is set (the hot path),
each noisy layer is ONE fused kernel call (ops.fused_noisy_conv2d /
fused_noisy_linear: MFMA implicit-GEMM with dual accumulators computing the
clean output and the sigma-conv from the same input tiles, Gaussian noise
sampled in-kernel) and pool/BN/ReLU/clip run as fused epilogue kernels.
The introspective path (plot/merge_bn/L2_act*/print_stats/train_act_max)
falls back to the compositional ops to expose every intermediate the
reference exposes (model.conv1_, model.relu1_, ...).

conv1 + its max-pool: in steady state (telemetry off, i >= 20) with no
double-backward penalty (L3/L3_new/L4 == 0) the hot path runs conv1, its
noise and the 2x2 max-pool as ONE kernel (ops.fused_noisy_conv2d_pool: the
im2col rows are gathered in-kernel, the pool happens in registers) and the
backward as one un-pool + wgrad kernel. The forward is bit-identical to the
two-op composition, so the switch at iteration 20 is invisible. On that path
the un-pooled activation never exists and ``model.conv1_`` is None; only the
introspective path and the L2_act/L3_act penalties read it, and those never
take the fused-pool path. NOISYNET_NO_CONV1_POOL=1 selects the composition.

bn1 -> relu -> clip -> quantize2 -> conv2: in steady state (training, 16-bit
on the GPU, single-rank BN, no conv dropout, q_a2 > 0, current2 > 0, no
crossbar mode, i >= 20, quantize2 calibrated to a fixed range from 0) the hot
path runs ops.bn_act_quant: after the BN statistics ONE kernel reads the
pooled conv1 output and writes the activation (for the backward kernels), the
quantised activation already channel-padded the way conv2's kernel stages it,
and its maximum (conv2's input_max). The unpadded quantised tensor of the
composition (bn_act -> fake_quant -> max -> pad) is never stored; the backward
is the composition's own. Values, gradients, running statistics, the seed
sequence and quantize2.last_range are bit-identical to the composition, which
every other case takes unchanged; NOISYNET_NO_BN_QUANT_FUSE=1 forces it.

Tiled crossbars (--xbar_rows N > 0): every layer's contraction is cut into
blocks of N crossbar rows (the (r, s, c) filter order; the input index for a
linear layer), each with its own current noise (if the layer's current > 0)
and its own ADC (--q_adc bits over +-adc_max), through ops.xbar_noisy_conv2d /
xbar_noisy_linear on the hot path. The conv1+pool kernel is bypassed, the
introspective flags are refused (ValueError), and ``model.adc_clip`` /
``model.partial_absmax`` collect the first 20 batches' ADC statistics next to
power / nsr. With --xbar_rows 0 nothing changes. --xbar_diff puts W+ and W- of
every tile on two columns, each with its own noise and a unipolar ADC over
[0, adc_max] (ops.xbar_noisy_*(..., differential=True)); ``adc_clip`` is then
the share of clipped COLUMN partials. It needs --xbar_rows.

Bit-serial inputs (--xbar_dac_bits D > 0, with --xbar_rows): every crossbar
layer streams its q_a<k>-bit activation code D bits per cycle, J = ceil(q_a/D)
<= 4 slices, each slice of each tile with its own noise draw and its own ADC
conversion, shift-added digitally (ops.xbar_noisy_*(..., in_bits, dac_bits,
x_step)). The activation LSB x_step = max((max - min) / (2^q_a - 1), 1e-6)
comes from the range the preceding QuantMeasure quantised with (its
``last_range``), so every layer needs q_a<k> > 0 and a range that starts at 0.
--adc_max is then the range of one SLICE conversion and ``adc_clip`` /
``partial_absmax`` are per slice partial. The layer's noise factor is
unchanged (same cell current per unit input), so the MSB slice's noise enters
the output times 2^((J-1)D). Not combinable with --xbar_diff; bf16 carries at
most 7-bit codes. With --xbar_dac_bits 0 nothing changes.

Bit-sliced weights (--xbar_cell_bits E in 1..4, with --xbar_rows): a cell
holds E bits, so every crossbar layer spreads its q_w<k>-bit weight code over
T = ceil(q_w/E) <= 4 columns (ops.xbar_noisy_*(..., w_bits, cell_bits, w_step,
w_min)). The code is offset binary on the grid of the layer's weight quantiser,
w = w_min + code * w_step with w_step = max((hi - lo) / (2^q_w - 1), 1e-6) and
w_min = lo from its ``last_range``. Per tile b and slice t
    p_bt = w_step * sum x * d_t              d_t = (code >> tE) & (2^E - 1)
    v_bt = p_bt + eps_bt * sqrt(factor * s_bt),  s_bt = sum x * f(w_step * d_t)
    q_bt = unipolar ADC of v_bt over [0, adc_max]
    out  = sum_b (sum_t 2^(tE) q_bt + w_min * sum x) + bias
Two consequences: offset-binary cells carry current even for a zero weight
(code -w_min / w_step), so noise and power are higher than the signed
one-cell model's; and --adc_max is a per-slice, unipolar figure, to be read
off the printed max |partial| (``adc_clip`` / ``partial_absmax`` are per cell
slice partial). Every layer needs 0 < q_w<k> < 8 (NoisyLinear leaves 8-bit
weights unquantised) and a range whose codes the dtype carries:
max(|lo|, |hi|) * u_dtype < w_step / 2. Not combinable with --xbar_diff,
--xbar_dac_bits or the introspective flags. With --xbar_cell_bits 0 nothing
changes.

Programmed cells (--xbar_cell_var sigma, --xbar_cell_stuck_off p,
--xbar_cell_stuck_on p, --xbar_cell_seed S; with --xbar_cell_bits): the cells
of the bit-sliced arrays hold imperfect conductances. Each crossbar layer
programs its weight codes once (ops.xbar_program_cells, one HIP launch) into
G[T, K, n] and the fused op reads G in place of the ideal digits
(ops.xbar_noisy_*(..., cells=G)). Per cell, one (u, z) Philox draw keyed by
the chip seed, counter (t*K + k)*n + i:
    d'_t = 0 if u < p_off (stuck at the high-resistance state),
           2^E - 1 else if u < p_off + p_on (stuck on), else d_t
    G_t  = round_to_dtype(max(d'_t * (1 + sigma * z), 0))      (digit units)
    p_bt = w_step * sum x * G_t
    s_bt = max(p_bt, 0) (abs),  max(w_step^2 * sum x * G_t^2 + p_bt, 0) (abs2)
and v_bt, the ADC, the shift-add and the exact digital offset w_min * sum x
are those of the bit-sliced model. The variation is multiplicative and
Gaussian, clamped at zero (an off cell stays off; a stuck-on cell varies like
any other); log-normal variation and additive HRS leakage are not modelled. A
fault in the MSB slice enters the output times 2^((T-1)E), which editing the
weights cannot express. Gradients stay those of the plain layer on wq.
Schedule: in training mode a layer programs its cells on every forward (the
weights change); in eval mode once per weight version -- the cache is keyed on
the weight parameter's ``_version`` / ``data_ptr`` (the effective weight is a
fresh tensor per forward, derived from it), the quantiser's range, the dtype
and the cell arguments, and is dropped on ``train()`` / ``eval()``. So one
evaluation sees one chip. --xbar_cell_seed -1 (default) draws a fresh chip at
every programming, so repeated evaluations see different chips; S >= 0 is one
fixed chip, layer k (0..3) using seed 4*S + k. With all three rates 0 nothing
changes: no cell is programmed and the op runs on the digits.
"""

import torch
from torch import nn

from .. import ops
from ..config import xbar_cell_model
from ..hardware_model import NoisyConv2d, NoisyLinear, add_noise_calculate_power
from ..quant import QuantMeasure


class Net(nn.Module):
    def __init__(self, args=None):
        super().__init__()
        self.args = args
        self.create_dir = True

        if args.train_act_max:
            self.act_max1 = nn.Parameter(torch.Tensor([0]), requires_grad=True)
            self.act_max2 = nn.Parameter(torch.Tensor([0]), requires_grad=True)
            self.act_max3 = nn.Parameter(torch.Tensor([0]), requires_grad=True)
        if args.train_w_max:
            self.w_max1 = nn.Parameter(torch.Tensor([0]), requires_grad=True)
            self.w_min1 = nn.Parameter(torch.Tensor([0]), requires_grad=True)

        self.pool = nn.MaxPool2d(2, 2)
        self.relu = nn.ReLU()

        self.quantize1 = QuantMeasure(args.q_a1, stochastic=args.stochastic,
                                      pctl=args.pctl, max_value=1.0,
                                      debug=args.debug_quant)
        self.quantize2 = QuantMeasure(args.q_a2, stochastic=args.stochastic,
                                      pctl=args.pctl, debug=args.debug_quant)
        self.quantize3 = QuantMeasure(args.q_a3, stochastic=args.stochastic,
                                      pctl=args.pctl,
                                      max_value=args.act_max / (1. - args.dropout),
                                      debug=args.debug_quant)
        self.quantize4 = QuantMeasure(args.q_a4, stochastic=args.stochastic,
                                      pctl=args.pctl, debug=args.debug_quant)

        fm1, fm2 = args.fm1 * args.width, args.fm2 * args.width
        fc = args.fc * args.width
        self.conv1 = NoisyConv2d(3, fm1, kernel_size=args.fs, bias=args.use_bias,
                                 num_bits=0, num_bits_weight=args.q_w1,
                                 noise=args.n_w1, test_noise=args.n_w_test,
                                 stochastic=args.stochastic, debug=args.debug_noise)
        self.conv2 = NoisyConv2d(fm1, fm2, kernel_size=args.fs, bias=args.use_bias,
                                 num_bits=0, num_bits_weight=args.q_w2,
                                 noise=args.n_w2, test_noise=args.n_w_test,
                                 stochastic=args.stochastic, debug=args.debug_noise)
        self.linear1 = NoisyLinear(fm2 * args.fs * args.fs, fc, bias=args.use_bias,
                                   num_bits=0, num_bits_weight=args.q_w3,
                                   noise=args.n_w3, test_noise=args.n_w_test,
                                   stochastic=args.stochastic, debug=args.debug_noise)
        self.linear2 = NoisyLinear(fc, 10, bias=args.use_bias,
                                   num_bits=0, num_bits_weight=args.q_w4,
                                   noise=args.n_w4, test_noise=args.n_w_test,
                                   stochastic=args.stochastic, debug=args.debug_noise)

        if args.batchnorm:
            self.bn1 = nn.BatchNorm2d(fm1, track_running_stats=args.track_running_stats)
            self.bn2 = nn.BatchNorm2d(fm2, track_running_stats=args.track_running_stats)
            if args.bn3:
                self.bn3 = nn.BatchNorm1d(fc, track_running_stats=args.track_running_stats)
            if args.bn4:
                self.bn4 = nn.BatchNorm1d(10, track_running_stats=args.track_running_stats)

        if args.dropout > 0:
            self.dropout = nn.Dropout(p=args.dropout)

        # telemetry lists (reset per epoch by the driver)
        self.power = [[] for _ in range(args.num_layers)]
        self.nsr = [[] for _ in range(args.num_layers)]
        self.input_sparsity = [[] for _ in range(args.num_layers)]
        # tiled crossbars (--xbar_rows): share of clipped tile partials and
        # max |tile partial| per layer, first 20 batches like power / nsr
        self.adc_clip = [[] for _ in range(args.num_layers)]
        self.partial_absmax = [[] for _ in range(args.num_layers)]
        self.xbar_rows = getattr(args, 'xbar_rows', 0) or 0
        self.xbar_diff = bool(getattr(args, 'xbar_diff', False))
        if self.xbar_diff and self.xbar_rows <= 0:
            raise ValueError('--xbar_diff needs --xbar_rows > 0: differential '
                             'columns are a mode of the tiled crossbars')
        self.xbar_dac_bits = getattr(args, 'xbar_dac_bits', 0) or 0
        if self.xbar_dac_bits > 0 and self.xbar_rows <= 0:
            raise ValueError('--xbar_dac_bits needs --xbar_rows > 0: bit-serial '
                             'inputs are a mode of the tiled crossbars')
        self.xbar_cell_bits = getattr(args, 'xbar_cell_bits', 0) or 0
        if self.xbar_cell_bits > 0 and self.xbar_rows <= 0:
            raise ValueError('--xbar_cell_bits needs --xbar_rows > 0: '
                             'bit-sliced weights are a mode of the tiled '
                             'crossbars')
        self._cells_cache = {}
        xbar_cell_model(args)     # the --xbar_cell_* flags, with or without
        if self.xbar_rows > 0:    # --xbar_rows
            self._check_xbar_args()

    def train(self, mode=True):
        # programmed cells are cached in eval mode only, for one evaluation
        self._cells_cache = {}
        return super().train(mode)

    # ------------------------------------------------------------------
    _INTROSPECTIVE_BOOLS = ('plot', 'write', 'merge_bn', 'distort_act',
                            'print_stats', 'train_act_max')
    _INTROSPECTIVE_FLOATS = ('L2_act1', 'L2_act2', 'L2_act3', 'L2_act4',
                             'L3_act', 'uniform_ind', 'uniform_dep',
                             'normal_ind', 'normal_dep')

    def _introspective_flags(self):
        a = self.args
        return [n for n in self._INTROSPECTIVE_BOOLS if getattr(a, n)] \
            + [n for n in self._INTROSPECTIVE_FLOATS if getattr(a, n) > 0]

    def _introspective(self):
        return bool(self._introspective_flags())

    def _check_xbar_args(self):
        a = self.args
        q_adc = getattr(a, 'q_adc', 0) or 0
        adc_max = [getattr(a, 'adc_max%d' % k, 0.0) for k in (1, 2, 3, 4)]
        if self.xbar_rows % 32:
            raise ValueError('--xbar_rows must be a positive multiple of 32, '
                             'got %d' % self.xbar_rows)
        if not (q_adc == 0 or 2 <= q_adc <= 16):
            raise ValueError('--q_adc must be 0 or 2..16, got %d' % q_adc)
        if q_adc > 0 and not all(m > 0 for m in adc_max):
            raise ValueError('--q_adc > 0 needs --adc_max (or every '
                             '--adc_max1..4) > 0, got %s' % adc_max)
        D = self.xbar_dac_bits = getattr(a, 'xbar_dac_bits', 0) or 0
        if D < 0:
            raise ValueError('--xbar_dac_bits must be >= 0, got %d' % D)
        if D > 0:
            if self.xbar_diff:
                raise ValueError('--xbar_dac_bits cannot be combined with '
                                 '--xbar_diff: differential columns with '
                                 'bit-serial inputs are not built')
            for k in (1, 2, 3, 4):
                q_a = getattr(a, 'q_a%d' % k)
                if q_a <= 0:
                    raise ValueError(
                        '--xbar_dac_bits needs a quantised input on every '
                        'layer: --q_a%d is 0' % k)
                if q_a > 8 or (q_a == 8 and getattr(a, 'bf16', False)):
                    raise ValueError(
                        '--xbar_dac_bits: --q_a%d %d is too wide; activation '
                        'codes have at most 8 bits, 7 with --bf16 (bf16 does '
                        'not carry every 8-bit code)' % (k, q_a))
                if -(-q_a // D) > 4:
                    raise ValueError(
                        '--xbar_dac_bits %d cuts --q_a%d %d into %d slices, at '
                        'most 4 are built; the smallest --xbar_dac_bits that '
                        'works is %d' % (D, k, q_a, -(-q_a // D),
                                         -(-q_a // 4)))
        E = self.xbar_cell_bits = getattr(a, 'xbar_cell_bits', 0) or 0
        if E < 0 or E > 4:
            raise ValueError('--xbar_cell_bits must be 0 or 1..4, got %d' % E)
        if E > 0:
            if self.xbar_diff or D > 0:
                raise ValueError(
                    '--xbar_cell_bits cannot be combined with --%s: T * J '
                    'accumulator sets per output do not fit the kernel, and '
                    'W+ / W- columns per weight slice are a follow-up'
                    % ('xbar_diff' if self.xbar_diff else 'xbar_dac_bits'))
            for k in (1, 2, 3, 4):
                q_w = getattr(a, 'q_w%d' % k)
                if not 0 < q_w < 8:
                    raise ValueError(
                        '--xbar_cell_bits needs quantised weights on every '
                        'layer, 0 < q_w < 8 (8-bit weights of a linear layer '
                        'stay unquantised): --q_w%d is %d' % (k, q_w))
                if -(-q_w // E) > 4:
                    raise ValueError(
                        '--xbar_cell_bits %d cuts --q_w%d %d into %d slices, '
                        'at most 4 are built; the smallest --xbar_cell_bits '
                        'that works is %d' % (E, k, q_w, -(-q_w // E),
                                              -(-q_w // 4)))
        xbar_cell_model(a)
        flags = self._introspective_flags()
        if flags:
            raise ValueError(
                '--xbar_rows %d cannot be combined with --%s: that flag runs '
                'the introspective forward, which models one unbounded '
                'crossbar per layer' % (self.xbar_rows, flags[0]))

    def _conv1_pool_fused(self, x, i):
        """conv1 and its max-pool run as one kernel (see module docstring)."""
        a = self.args
        return (a.current1 > 0 and i >= 20 and not x.requires_grad
                and a.L3 == 0 and a.L4 == 0
                and getattr(a, 'L3_new', 0) == 0
                and ops.conv_pool_eligible(x, self.conv1.weight))

    def _bn_quant_range(self, x, i):
        """quantize2's (min, max, stochastic) when bn1 + quantize2 + conv2 run
        through ops.bn_act_quant (see module docstring), else None."""
        import os
        a = self.args
        if not (self.training and a.batchnorm and i >= 20
                and self.xbar_rows == 0 and a.q_a2 > 0 and a.current2 > 0
                and a.dropout_conv == 0
                and not getattr(a, 'sync_bn', False)
                and not self.quantize2.calculate_running
                and not os.environ.get('NOISYNET_NO_BN_QUANT_FUSE')
                and ops.bn_act_quant_native(x, self.bn1.running_mean, 0.0)):
            return None
        rng = self.quantize2.quant_range()
        if rng is None or rng[0] != 0:
            return None
        return rng

    def _noisy_layer_fused(self, x, layer, current, merged_dac, i, layer_num,
                           is_conv, pool=False, x_pad=None, input_max=None):
        """One fused pass: quantized-weight conv/GEMM + sigma + noise
        (+ the following 2x2 max-pool when ``pool``). ``x_pad`` / ``input_max``
        come from ops.bn_act_quant: the channel-padded input the conv runs on
        and max(x), which is then not reduced again."""
        a = self.args
        w_raw = layer.weight
        wq, bias = layer.effective_weight()
        want_telemetry = i < 20
        with torch.no_grad():
            # input_max is a full-tensor reduce over the activation; for
            # merged-DAC layers it only feeds the power telemetry
            # (first-20-batch), so skip it in steady state
            if merged_dac:
                w_max = w_raw.detach().abs().max()
                factor = 0.1 * w_max / current
                sigma_mode = 'abs'
                power_denom = (x.detach().max() * w_max if want_telemetry
                               else w_max)
            else:
                if input_max is None:
                    input_max = x.detach().max()
                factor = 0.1 * input_max / current
                sigma_mode = 'abs2'
                power_denom = input_max
        telem = ops.NoiseTelemetry() if want_telemetry else None
        if is_conv:
            conv = ops.fused_noisy_conv2d_pool if pool \
                else ops.fused_noisy_conv2d
            extra = {} if x_pad is None else {'x_pad': x_pad}
            out = conv(
                x, wq, w_raw.detach(), bias, 1, 0, sigma_mode, factor,
                current=current, power_denom=power_denom,
                want_telemetry=want_telemetry, telemetry_out=telem, **extra)
        else:
            out = ops.fused_noisy_linear(
                x, wq, w_raw.detach(), bias, sigma_mode, factor,
                current=current, power_denom=power_denom,
                want_telemetry=want_telemetry, telemetry_out=telem)
        if want_telemetry and telem.power is not None:
            self.power[layer_num].append(float(telem.power))
            self.nsr[layer_num].append(float(telem.nsr))
            self.input_sparsity[layer_num].append(float(telem.input_sparsity))
        return out

    def _xbar_serial_args(self, layer_num):
        """in_bits / dac_bits / x_step of a layer under --xbar_dac_bits: the
        code width is the layer's q_a, the LSB that of the range its
        QuantMeasure has just quantised with."""
        if self.xbar_dac_bits <= 0:
            return {}
        k = layer_num + 1
        q_a = getattr(self.args, 'q_a%d' % k)
        lo, hi = getattr(self, 'quantize%d' % k).last_range
        if lo != 0:
            raise ValueError(
                '--xbar_dac_bits: quantize%d has the range minimum %g; '
                'bit-serial inputs need unsigned codes (a range from 0)'
                % (k, lo))
        return dict(in_bits=q_a, dac_bits=self.xbar_dac_bits,
                    x_step=max((hi - lo) / (2.0 ** q_a - 1.0), 1e-6))

    def _xbar_cell_args(self, layer_num, layer, dtype):
        """w_bits / cell_bits / w_step / w_min of a layer under
        --xbar_cell_bits: the code width is the layer's q_w, the grid that of
        the range its weight quantiser has just quantised with. Decided from
        the range's floats alone (no device read)."""
        if self.xbar_cell_bits <= 0:
            return {}
        k = layer_num + 1
        q_w = getattr(self.args, 'q_w%d' % k)
        lo, hi = layer.quantize_weights.last_range
        w_step = max((hi - lo) / (2.0 ** q_w - 1.0), 1e-6)
        # one rounding to the dtype moves a grid weight by at most
        # max|w| * u; the code is recovered while that stays below half a step
        u = torch.finfo(dtype).eps / 2
        if max(abs(lo), abs(hi)) * u >= w_step / 2:
            raise ValueError(
                '--xbar_cell_bits: the %d-bit weight codes of layer %d on the '
                'range [%g, %g] (step %g) cannot be recovered from %s weights'
                % (q_w, k, lo, hi, w_step, dtype))
        return dict(w_bits=q_w, cell_bits=self.xbar_cell_bits, w_step=w_step,
                    w_min=lo)

    def _xbar_cells(self, layer_num, layer, wq, cell_args):
        """The layer's programmed conductances G under --xbar_cell_var /
        --xbar_cell_stuck_*, or None for ideal cells. Training programs on
        every forward; eval once per weight version (see module docstring)."""
        model = xbar_cell_model(self.args)
        if model is None or not cell_args:
            return None
        sigma, p_off, p_on, seed = model
        chip = None if seed < 0 else 4 * seed + layer_num
        kw = dict(sigma=sigma, p_stuck_off=p_off, p_stuck_on=p_on, seed=chip)
        if self.training:
            return ops.xbar_program_cells(wq, **cell_args, **kw)
        w = layer.weight
        key = (w._version, w.data_ptr(), wq.dtype, wq.device,
               tuple(sorted(cell_args.items())), sigma, p_off, p_on, seed)
        hit = self._cells_cache.get(layer_num)
        if hit is None or hit[0] != key:
            hit = (key, ops.xbar_program_cells(wq, **cell_args, **kw))
            self._cells_cache[layer_num] = hit
        return hit[1]

    def _xbar_layer(self, x, layer, current, merged_dac, i, layer_num,
                    is_conv):
        """The layer on tiled crossbars: per-tile noise when its current is
        > 0 and per-tile ADC when --q_adc > 0 (ops.xbar_noisy_*). A layer with
        neither is the plain layer, which tiling does not change. With
        --xbar_diff every tile runs on differential columns, with
        --xbar_dac_bits on bit-serial inputs."""
        a = self.args
        q_adc = getattr(a, 'q_adc', 0) or 0
        if current <= 0 and q_adc == 0:
            return layer(x)
        adc_max = getattr(a, 'adc_max%d' % (layer_num + 1), 0.0)
        w_raw = layer.weight
        wq, bias = layer.effective_weight()
        want_telemetry = i < 20
        sigma_mode, factor, power_denom = None, 0.0, 1.0
        if current > 0:
            with torch.no_grad():
                if merged_dac:
                    w_max = w_raw.detach().abs().max()
                    factor = 0.1 * w_max / current
                    sigma_mode = 'abs'
                    power_denom = (x.detach().max() * w_max if want_telemetry
                                   else w_max)
                else:
                    input_max = x.detach().max()
                    factor = 0.1 * input_max / current
                    sigma_mode = 'abs2'
                    power_denom = input_max
        telem = ops.XbarTelemetry() if want_telemetry else None
        serial = self._xbar_serial_args(layer_num)
        cell_args = self._xbar_cell_args(layer_num, layer, wq.dtype)
        serial.update(cell_args)
        cells = self._xbar_cells(layer_num, layer, wq, cell_args)
        if cells is not None:
            serial['cells'] = cells
        if is_conv:
            out = ops.xbar_noisy_conv2d(
                x, wq, w_raw.detach(), bias, 1, 0, sigma_mode, factor,
                self.xbar_rows, q_adc, adc_max, current=current,
                power_denom=power_denom, want_telemetry=want_telemetry,
                telemetry_out=telem, differential=self.xbar_diff, **serial)
        else:
            out = ops.xbar_noisy_linear(
                x, wq, w_raw.detach(), bias, sigma_mode, factor,
                self.xbar_rows, q_adc, adc_max, current=current,
                power_denom=power_denom, want_telemetry=want_telemetry,
                telemetry_out=telem, differential=self.xbar_diff, **serial)
        if want_telemetry:
            if telem.power is not None:
                self.power[layer_num].append(float(telem.power))
                self.nsr[layer_num].append(float(telem.nsr))
                self.input_sparsity[layer_num].append(
                    float(telem.input_sparsity))
            self.adc_clip[layer_num].append(float(telem.adc_clip_share))
            self.partial_absmax[layer_num].append(float(telem.partial_absmax))
        return out

    def _bn_act(self, x, bn, act_max):
        """Fused BN + ReLU + clip."""
        return ops.bn_act(x, bn.weight, bn.bias, bn.running_mean,
                          bn.running_var,
                          self.training or not self.args.track_running_stats,
                          bn.momentum, bn.eps, relu=True, act_max=act_max,
                          sync=getattr(self.args, 'sync_bn', False))

    # ------------------------------------------------------------------
    def forward(self, input, epoch=0, i=0, s=0, acc=0.0):
        args = self.args
        if self.xbar_rows > 0:
            self._check_xbar_args()   # args may have changed since __init__
            return self._forward_fused(input, i)
        if not self._introspective():
            return self._forward_fused(input, i)
        return self._forward_reference(input, epoch, i, s, acc)

    # -- the hot path ---------------------------------------------------
    def _forward_fused(self, input, i=0):
        args = self.args

        x = self.quantize1(input) if args.q_a1 > 0 else input
        self.input = x

        xbar = self.xbar_rows > 0
        if xbar:
            # tiled crossbars bypass the conv1+pool single-kernel route
            x = self._xbar_layer(x, self.conv1, args.current1,
                                 args.merged_dac, i, 0, True)
            self.conv1_ = x
            x = ops.maxpool2x2(x)
        elif self._conv1_pool_fused(x, i):
            x = self._noisy_layer_fused(x, self.conv1, args.current1,
                                        args.merged_dac, i, 0, True, pool=True)
            self.conv1_ = None
        else:
            if args.current1 > 0:
                x = self._noisy_layer_fused(x, self.conv1, args.current1,
                                            args.merged_dac, i, 0, True)
            else:
                x = self.conv1(x)
            self.conv1_ = x
            x = ops.maxpool2x2(x)
        q2 = self._bn_quant_range(x, i)
        if q2 is not None:
            # bn1 + relu + clip + quantize2 (+ conv2's channel padding and
            # input_max) as one kernel each way
            bn = self.bn1
            x, x_pad, x_max = ops.bn_act_quant(
                x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                bn.momentum, bn.eps, args.act_max1, args.q_a2, q2[0], q2[1],
                q2[2], c_pad=ops.conv_input_pad_width(x, self.conv2.weight))
            x = self._noisy_layer_fused(x, self.conv2, args.current2, False,
                                        i, 1, True, x_pad=x_pad,
                                        input_max=x_max)
        else:
            if args.batchnorm:
                x = self._bn_act(x, self.bn1, args.act_max1)
            else:
                x = ops.relu_clip(x, args.act_max1)
            if args.dropout_conv > 0:
                x = ops.dropout(x, args.dropout_conv, self.training)
            if args.q_a2 > 0:
                x = self.quantize2(x)

        if q2 is not None:
            pass
        elif xbar:
            x = self._xbar_layer(x, self.conv2, args.current2, False, i, 1,
                                 True)
        elif args.current2 > 0:
            x = self._noisy_layer_fused(x, self.conv2, args.current2,
                                        False, i, 1, True)
        else:
            x = self.conv2(x)
        self.conv2_ = x
        x = ops.maxpool2x2(x)
        if args.batchnorm:
            x = self._bn_act(x, self.bn2, args.act_max2)
        else:
            x = ops.relu_clip(x, args.act_max2)
        if args.dropout > 0:
            x = ops.dropout(x, args.dropout, self.training)

        x = x.reshape(x.size(0), -1)
        if args.q_a3 > 0:
            x = self.quantize3(x)

        if xbar:
            x = self._xbar_layer(x, self.linear1, args.current3,
                                 args.merged_dac, i, 2, False)
        elif args.current3 > 0:
            x = self._noisy_layer_fused(x, self.linear1, args.current3,
                                        args.merged_dac, i, 2, False)
        else:
            x = self.linear1(x)
        self.linear1_ = x
        if args.batchnorm and args.bn3:
            x = self._bn_act(x, self.bn3, args.act_max3)
        else:
            x = ops.relu_clip(x, args.act_max3)
        if args.dropout > 0:
            x = ops.dropout(x, args.dropout, self.training)
        if args.q_a4 > 0:
            x = self.quantize4(x)

        if xbar:
            x = self._xbar_layer(x, self.linear2, args.current4, False, i, 3,
                                 False)
        elif args.current4 > 0:
            x = self._noisy_layer_fused(x, self.linear2, args.current4,
                                        False, i, 3, False)
        else:
            x = self.linear2(x)
        self.linear2_ = x
        if args.batchnorm and args.bn4:
            x = ops.bn_act(x, self.bn4.weight, self.bn4.bias,
                           self.bn4.running_mean, self.bn4.running_var,
                           self.training or not args.track_running_stats,
                           self.bn4.momentum, self.bn4.eps,
                           relu=False, act_max=0.0,
                           sync=getattr(args, 'sync_bn', False))
        self.linear2_out = x
        return x

    # -- the introspective path (exact reference op order + attributes) --
    def _forward_reference(self, input, epoch=0, i=0, s=0, acc=0.0):
        args = self.args
        arrays = []

        if args.q_a1 > 0:
            self.input = self.quantize1(input)
        else:
            self.input = input

        self.conv1_no_bias = self.conv1(self.input)

        if args.merge_bn:
            self.bias1 = (self.bn1.bias.view(1, -1, 1, 1)
                          - self.bn1.running_mean.data.view(1, -1, 1, 1)
                          * self.bn1.weight.data.view(1, -1, 1, 1)
                          / torch.sqrt(self.bn1.running_var.data.view(1, -1, 1, 1) + 1e-7))
            self.conv1_ = self.conv1_no_bias + self.bias1
        else:
            self.conv1_ = self.conv1_no_bias

        if args.current1 > 0 or args.distort_act:
            conv1_out = add_noise_calculate_power(
                self, args, arrays, self.input, self.conv1.weight, self.conv1_,
                layer_type='conv', i=i, layer_num=0, merged_dac=args.merged_dac)
        else:
            conv1_out = self.conv1_

        pool1 = self.pool(conv1_out)
        if args.batchnorm and not args.merge_bn:
            self.pool1_out = self.bn1(pool1)
        else:
            self.pool1_out = pool1

        self.relu1_ = self.relu(self.pool1_out)
        if args.act_max1 > 0:
            if args.train_act_max:
                self.relu1_clipped = torch.where(self.relu1_ > self.act_max1,
                                                 self.act_max1, self.relu1_)
            else:
                self.relu1_clipped = torch.clamp(self.relu1_, max=args.act_max1)
            self.relu1 = self.relu1_clipped
        else:
            self.relu1 = self.relu1_

        if args.L3_act > 0:
            self.relu1_.retain_grad()
            self.relu1.retain_grad()
        if args.train_act_max:
            self.relu1_clipped.retain_grad()
        if args.train_w_max:
            self.w_max1.retain_grad()
            self.w_min1.retain_grad()

        if args.dropout_conv > 0:
            self.relu1 = self.dropout(self.relu1)
        if args.q_a2 > 0:
            self.relu1 = self.quantize2(self.relu1)

        self.conv2_no_bias = self.conv2(self.relu1)
        if args.merge_bn:
            self.bias2 = (self.bn2.bias.view(1, -1, 1, 1)
                          - self.bn2.running_mean.data.view(1, -1, 1, 1)
                          * self.bn2.weight.data.view(1, -1, 1, 1)
                          / torch.sqrt(self.bn2.running_var.data.view(1, -1, 1, 1) + 1e-7))
            self.conv2_ = self.conv2_no_bias + self.bias2
        else:
            self.conv2_ = self.conv2_no_bias

        if args.current2 > 0 or args.distort_act:
            conv2_out = add_noise_calculate_power(
                self, args, arrays, self.relu1, self.conv2.weight, self.conv2_,
                layer_type='conv', i=i, layer_num=1, merged_dac=False)
        else:
            conv2_out = self.conv2_

        pool2 = self.pool(conv2_out)
        if args.batchnorm and not args.merge_bn:
            self.pool2_out = self.bn2(pool2)
        else:
            self.pool2_out = pool2

        self.relu2_ = self.relu(self.pool2_out)
        if args.act_max2 > 0:
            if args.train_act_max:
                self.relu2_clipped = torch.where(self.relu2_ > self.act_max2,
                                                 self.act_max2, self.relu2_)
            else:
                self.relu2_clipped = torch.clamp(self.relu2_, max=args.act_max2)
            self.relu2 = self.relu2_clipped
        else:
            self.relu2 = self.relu2_

        if args.L3_act > 0:
            self.relu2.retain_grad()
        if args.dropout > 0:
            self.relu2 = self.dropout(self.relu2)

        self.relu2 = self.relu2.reshape(self.relu2.size(0), -1)
        if args.q_a3 > 0:
            self.relu2 = self.quantize3(self.relu2)

        self.linear1_no_bias = self.linear1(self.relu2)
        if args.merge_bn:
            self.bias3 = (self.bn3.bias.view(1, -1)
                          - self.bn3.running_mean.data.view(1, -1)
                          * self.bn3.weight.data.view(1, -1)
                          / torch.sqrt(self.bn3.running_var.data.view(1, -1) + 1e-7))
            self.linear1_ = self.linear1_no_bias + self.bias3
        else:
            self.linear1_ = self.linear1_no_bias

        if args.current3 > 0 or args.distort_act:
            linear1_out = add_noise_calculate_power(
                self, args, arrays, self.relu2, self.linear1.weight,
                self.linear1_, layer_type='linear', i=i, layer_num=2,
                merged_dac=args.merged_dac)
        else:
            linear1_out = self.linear1_

        if args.batchnorm and args.bn3 and not args.merge_bn:
            self.linear1_out = self.bn3(linear1_out)
        else:
            self.linear1_out = linear1_out

        self.relu3_ = self.relu(self.linear1_out)
        if args.act_max3 > 0:
            if args.train_act_max:
                self.relu3_clipped = torch.where(self.relu3_ > self.act_max3,
                                                 self.act_max3, self.relu3_)
            else:
                self.relu3_clipped = torch.clamp(self.relu3_, max=args.act_max3)
            self.relu3 = self.relu3_clipped
        else:
            self.relu3 = self.relu3_

        if args.L3_act > 0:
            self.relu3.retain_grad()
        if args.dropout > 0:
            self.relu3 = self.dropout(self.relu3)
        if args.q_a4 > 0:
            self.relu3 = self.quantize4(self.relu3)

        self.linear2_no_bias = self.linear2(self.relu3)
        if args.bn4 and args.merge_bn:
            if self.training:
                raise RuntimeError('Merging BatchNorm during training!')
            self.bias4 = (self.bn4.bias.view(1, -1)
                          - self.bn4.running_mean.data.view(1, -1)
                          * self.bn4.weight.data.view(1, -1)
                          / torch.sqrt(self.bn4.running_var.data.view(1, -1) + 1e-7))
            self.linear2_ = self.linear2_no_bias + self.bias4
        else:
            self.linear2_ = self.linear2_no_bias
            self.bias4 = torch.Tensor([0])

        if args.current4 > 0 or args.distort_act:
            linear2_out = add_noise_calculate_power(
                self, args, arrays, self.relu3, self.linear2.weight,
                self.linear2_, layer_type='linear', i=i, layer_num=3,
                merged_dac=False)
        else:
            linear2_out = self.linear2_

        if args.batchnorm and args.bn4 and not args.merge_bn:
            self.linear2_out = self.bn4(linear2_out)
        else:
            self.linear2_out = linear2_out

        if args.plot or args.write:
            from .. import plot_histograms  # lazy; matplotlib is heavy
            plot_histograms.capture_and_emit(self, args, arrays, epoch, i, s, acc)

        return self.linear2_out


def noisynet(args):
    return Net(args)
