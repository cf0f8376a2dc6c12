"""Autograd-facing op layer with native (HIP/gfx950) vs reference dispatch.

Every hot op has two execution paths:
  * CUDA(ROCm) tensors -> the hand-written CDNA4 kernels in csrc/ (mandatory
    on GPU; a missing extension raises, never silently falls back), laid out
    NHWC (``torch.channels_last``) for convs.
  * CPU tensors -> ``noisynet_amd.ops.reference`` (pure PyTorch), which is
    also the oracle the GPU kernels are unit-tested against.

Autograd structure mirrors the reference semantics:
  * fake-quant uses a saturated STE (zero outside [min,max]) --
    hardware_model.py:175-183;
  * VMM noise is sampled under no_grad and added to the clean pre-activation,
    so gradients flow only through the clean conv/GEMM --
    hardware_model.py:23,125;
  * conv forward/dgrad/wgrad are mutually composable autograd Functions so
    the L3/L3_act/L4 gradient penalties (double/triple backward,
    noisynet.py:1348-1476) work through the custom kernels.
"""

import os as _os

import torch
import torch.nn.functional as F

from . import reference as ref
from ._ext import ext, use_native

# ---------------------------------------------------------------------------
# seeds for in-kernel Philox RNG: deterministic under torch.manual_seed
# ---------------------------------------------------------------------------

def _next_seed(device):
    # Draw from torch's generator so --seed reproduces kernel-side RNG too.
    return int(torch.randint(0, 2 ** 62, (1,), device="cpu").item())


# ---------------------------------------------------------------------------
# Fake quantization (UniformQuantize parity)
# ---------------------------------------------------------------------------


class FakeQuant(torch.autograd.Function):
    """Clamp-quantize-dequantize with stochastic rounding; saturated STE bwd."""

    @staticmethod
    def forward(ctx, x, num_bits, min_value, max_value, stochastic):
        ctx.min_value = float(min_value)
        ctx.max_value = float(max_value)
        ctx.save_for_backward(x)
        if use_native(x):
            return ext().fake_quant_fwd(
                x, int(num_bits), float(min_value), float(max_value),
                float(stochastic), _next_seed(x.device))
        return ref.fake_quant_forward(x, num_bits, min_value, max_value, stochastic)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        if use_native(x):
            # ste_mask aligns layouts internally (x.suggest_memory_format);
            # a plain .contiguous() here would force an NCHW round-trip
            g = ext().ste_mask(grad_output, x, ctx.min_value, ctx.max_value)
        else:
            g = ref.fake_quant_backward(grad_output, x, ctx.min_value, ctx.max_value)
        return g, None, None, None, None


def fake_quant(x, num_bits, min_value, max_value, stochastic=0.0):
    return FakeQuant.apply(x, num_bits, min_value, max_value, stochastic)



def _factor_tensor(f, device):
    """Noise factor as a device-resident f32 scalar (no host sync)."""
    if isinstance(f, torch.Tensor):
        return f.detach().to(device=device, dtype=torch.float32).reshape(1)
    return torch.tensor([float(f)], device=device, dtype=torch.float32)


# ---------------------------------------------------------------------------
# Conv primitives: forward / dgrad / wgrad, each differentiable by composition
# ---------------------------------------------------------------------------


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _patch_eligible(x, w, padding):
    """Mirror of csrc patch_eligible: image-resident LDS conv mode."""
    C = x.shape[1]
    R, S = w.shape[2], w.shape[3]
    c_pad = (C + 7) // 8 * 8
    wp = x.shape[3] + 2 * padding
    eb = x.element_size()
    return (R * S > 1 and C > 8
            and x.shape[2] * wp * c_pad * eb + 128 <= 96 * 1024)


def _conv_fwd_raw(x, w, bias, stride, padding):
    if use_native(x, w):
        R, S = w.shape[2], w.shape[3]
        if _patch_eligible(x, w, padding):
            empty = torch.empty(0, device=x.device, dtype=x.dtype)
            zero_f = torch.zeros(1, device=x.device, dtype=torch.float32)
            y = ext().conv_fwd_fused(_nhwc(x), _nhwc(w), _nhwc(w), empty,
                                     stride, padding, 0, zero_f, 0, False)[0]
        else:
            y = ext().conv_fwd(_nhwc(x), _nhwc(w), stride, padding)
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        return y
    return F.conv2d(x, w, bias, stride, padding)


def _conv_dgrad_raw(g, w, stride, padding, x_shape):
    if use_native(g, w):
        R, S = w.shape[2], w.shape[3]
        if stride == 1 and _patch_eligible(g, w, R - 1 - padding):
            # dgrad(stride 1) == conv of g with the flipped/transposed
            # filter at full-correlation padding -> image-patch kernel
            w2 = _nhwc(w.flip((2, 3)).transpose(0, 1))
            empty = torch.empty(0, device=g.device, dtype=g.dtype)
            zero_f = torch.zeros(1, device=g.device, dtype=torch.float32)
            dx = ext().conv_fwd_fused(_nhwc(g), w2, w2, empty, 1,
                                      R - 1 - padding, 0, zero_f, 0, False)[0]
            return dx
        if R * S == 1 and stride == 1 and padding == 0:
            # pointwise dgrad IS a GEMM: dx[M,C] = g[M,K] @ W[K,C]
            gn = _nhwc(g)
            K = gn.shape[1]
            m = gn.shape[0] * gn.shape[2] * gn.shape[3]
            g2 = gn.permute(0, 2, 3, 1).reshape(m, K)
            dx = ext().linear_dgrad(g2.contiguous(),
                                    w.reshape(w.shape[0], w.shape[1]))
            return dx.view(gn.shape[0], gn.shape[2], gn.shape[3],
                           w.shape[1]).permute(0, 3, 1, 2).contiguous(
                               memory_format=torch.channels_last)
        return ext().conv_dgrad(_nhwc(g), _nhwc(w), stride, padding,
                                x_shape[2], x_shape[3])
    return torch.nn.grad.conv2d_input(x_shape, w, g, stride, padding)


def _is_padded_input(shared, x):
    """Whether the tensor a fused forward handed back for sharing is the
    [N*H*W, round8(C)] channel-padded copy of x (conv_fwd_fused's noisy patch
    route) and not a flat im2col matrix, whose rows are at least 2*C wide."""
    C = x.shape[1]
    return (shared is not None and shared.dim() == 2 and C % 8 != 0
            and shared.shape[0] == x.shape[0] * x.shape[2] * x.shape[3]
            and shared.shape[1] == (C + 7) // 8 * 8)


def _conv_wgrad_raw(g, x, stride, padding, w_shape, col=None):
    if use_native(g, x):
        R, S = w_shape[2], w_shape[3]
        if _is_padded_input(col, x):
            # the noisy patch forward already padded x's channels to 8 (or
            # bn_act_quant wrote them padded): x gives the shape only, and
            # may be a strided view of that padded buffer
            return ext().conv_wgrad_patch(_nhwc(g), x, stride,
                                          padding, R, S, col)
        if col is not None and R * S > 1 \
                and not _os.environ.get("NOISYNET_WGRAD_NO_COL"):
            # flat im2col matrix shared from the forward pass
            return ext().conv_wgrad_from_col(_nhwc(g), col, x.shape[1], R, S)
        if R * S > 1 and x.element_size() == 2:
            # patch wgrad: x operand gathered in-kernel from the NHWC
            # input -- no materialized im2col pass at all
            return ext().conv_wgrad_patch(_nhwc(g), _nhwc(x), stride,
                                          padding, R, S)
        if R * S == 1 and stride == 1 and padding == 0:
            # pointwise conv wgrad IS a GEMM wgrad: flat NHWC views into
            # the 128-deep pipelined mk kernels (the generic conv wgrad
            # kernel was 2 ms/step of MobileNetV2's expand/project convs)
            gn, xn = _nhwc(g), _nhwc(x)
            K = gn.shape[1]
            C_in = xn.shape[1]
            m = gn.shape[0] * gn.shape[2] * gn.shape[3]
            g2 = gn.permute(0, 2, 3, 1).reshape(m, K)
            x2 = xn.permute(0, 2, 3, 1).reshape(m, C_in)
            dw = ext().linear_wgrad(g2.contiguous(), x2.contiguous())
            return dw.view(K, C_in, 1, 1).contiguous(
                memory_format=torch.channels_last)
        if R * S > 1:
            # fp32: im2col-GEMM wgrad when the buffer is affordable (<2 GB)
            C_in = x.shape[1]
            cols_p = (R * S * C_in if C_in % 8 == 0
                      else (R * S * C_in + 31) // 32 * 32)
            m = g.shape[0] * g.shape[2] * g.shape[3]
            col_bytes = m * cols_p * x.element_size()
            if col_bytes <= 2 << 30:
                return ext().conv_wgrad_im2col(_nhwc(g), _nhwc(x), stride,
                                               padding, R, S)
        return ext().conv_wgrad(_nhwc(g), _nhwc(x), stride, padding, R, S)
    return torch.nn.grad.conv2d_weight(x, w_shape, g, stride, padding)


class ConvFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padding):
        ctx.stride, ctx.padding = stride, padding
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return _conv_fwd_raw(x, w, bias, stride, padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ConvDgrad.apply(g, w, ctx.stride, ctx.padding, x.shape)
        if ctx.needs_input_grad[1]:
            gw = ConvWgrad.apply(g, x, ctx.stride, ctx.padding, w.shape, None)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None


class ConvDgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, w, stride, padding, x_shape):
        ctx.stride, ctx.padding = stride, padding
        ctx.x_shape = tuple(x_shape)
        ctx.save_for_backward(g, w)
        return _conv_dgrad_raw(g, w, stride, padding, x_shape)

    @staticmethod
    def backward(ctx, gg):
        g, w = ctx.saved_tensors
        d_g = d_w = None
        if ctx.needs_input_grad[0]:
            d_g = ConvFwd.apply(gg, w, None, ctx.stride, ctx.padding)
        if ctx.needs_input_grad[1]:
            d_w = ConvWgrad.apply(g, gg, ctx.stride, ctx.padding, w.shape, None)
        return d_g, d_w, None, None, None


class ConvWgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, stride, padding, w_shape, col=None):
        ctx.stride, ctx.padding = stride, padding
        ctx.w_shape = tuple(w_shape)
        ctx.save_for_backward(g, x)
        return _conv_wgrad_raw(g, x, stride, padding, w_shape, col)

    @staticmethod
    def backward(ctx, gw):
        g, x = ctx.saved_tensors
        d_g = d_x = None
        if ctx.needs_input_grad[0]:
            d_g = ConvFwd.apply(x, gw, None, ctx.stride, ctx.padding)
        if ctx.needs_input_grad[1]:
            d_x = ConvDgrad.apply(g, gw, ctx.stride, ctx.padding, x.shape)
        return d_g, d_x, None, None, None, None


def conv2d(x, w, bias=None, stride=1, padding=0):
    if isinstance(stride, (tuple, list)):
        stride = stride[0]
    if isinstance(padding, (tuple, list)):
        padding = padding[0]
    return ConvFwd.apply(x, w, bias, stride, padding)


# ---------------------------------------------------------------------------
# Fused noisy conv / linear: y = x*Wq (+bias) + N(0, sqrt(factor * x*f(|W|)))
# ---------------------------------------------------------------------------


class NoiseTelemetry:
    """Per-call telemetry matching hardware_model.py:55-88 (first-20-batch
    power / NSR / input-sparsity statistics). Values are 0-dim tensors."""

    __slots__ = ("power", "nsr", "input_sparsity")

    def __init__(self, power=None, nsr=None, input_sparsity=None):
        self.power = power
        self.nsr = nsr
        self.input_sparsity = input_sparsity


class _FusedNoisyConv(torch.autograd.Function):
    """Fused conv + sigma-conv + Gaussian noise.

    Forward computes, in ONE pass over the input tiles on GPU (dual MFMA
    accumulators; csrc/conv_mfma.hip):
        y      = conv(x, wq) [+ bias]
        sigma  = conv(x, f(|w_raw|)),  f per sigma_mode ('abs' | 'abs2')
        out    = y + eps * sqrt(factor * sigma),  eps ~ N(0,1) in-kernel
    Gradients flow through y only (noise is a detached additive term):
    hardware_model.py:23 wraps all noise math in no_grad.

    ``x_pad``: the [N*H*W, round8(C)] channel-padded input that bn_act_quant
    wrote; the kernel runs on it as it is and ``x`` (a view of it) is read for
    its shape only, in forward and backward.
    """

    @staticmethod
    def forward(ctx, x, wq, w_raw, bias, stride, padding, sigma_mode, factor,
                want_telemetry, telemetry_out, current, power_denom,
                x_pad=None):
        ctx.stride, ctx.padding = stride, padding
        ctx.has_bias = bias is not None
        col = None
        if x_pad is not None and not use_native(x, wq):
            raise ValueError("fused_noisy_conv2d: x_pad is a GPU-route argument")
        if use_native(x, wq):
            y, tele, col = ext().conv_fwd_fused(
                x if x_pad is not None else _nhwc(x), _nhwc(wq), _nhwc(w_raw),
                bias if bias is not None else torch.empty(0, device=x.device, dtype=x.dtype),
                stride, padding, 1 if sigma_mode == "abs" else 2,
                _factor_tensor(factor, x.device), _next_seed(x.device),
                bool(want_telemetry), x_pad)
            if want_telemetry:
                sum_sigma_abs = tele[0] / x.shape[0]
                sum_abs_noise = tele[1] / y.numel()
                max_y = tele[2]
        else:
            y = F.conv2d(x, wq, bias, stride, padding)
            with torch.no_grad():
                sig = ref.sigma_conv2d(x.detach(), w_raw, sigma_mode, stride, padding)
                noise = ref.vmm_noise(sig, factor)
                if want_telemetry:
                    if sigma_mode == "abs":
                        sig_abs = sig
                    else:
                        sig_abs = ref.sigma_conv2d(x.detach(), w_raw, "abs", stride, padding)
                    sum_sigma_abs = sig_abs.sum(dim=(1, 2, 3)).mean()
                    sum_abs_noise = noise.abs().mean()
                    max_y = y.detach().max()
            y = y + noise
        if want_telemetry and telemetry_out is not None:
            with torch.no_grad():
                telemetry_out.power = 1.2e-6 * current * sum_sigma_abs / power_denom
                telemetry_out.nsr = sum_abs_noise / max_y
                telemetry_out.input_sparsity = (x.detach() > 0).sum() / x.numel()
        if col is not None and col.numel():
            # the small-C route materialized the flat im2col matrix, or the
            # patch route a channel-padded copy of x; keep it so backward's
            # wgrad skips the re-materialization
            ctx.save_for_backward(x, wq, col)
        else:
            ctx.save_for_backward(x, wq)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wq = ctx.saved_tensors[0], ctx.saved_tensors[1]
        col = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ConvDgrad.apply(g, wq, ctx.stride, ctx.padding, x.shape)
        if ctx.needs_input_grad[1]:
            gw = ConvWgrad.apply(g, x, ctx.stride, ctx.padding, wq.shape, col)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = g.sum(dim=(0, 2, 3))
        return (gx, gw, None, gb) + (None,) * 9


def fused_noisy_conv2d(x, wq, w_raw, bias, stride, padding, sigma_mode,
                       factor, current=0.0, power_denom=1.0,
                       want_telemetry=False, telemetry_out=None, x_pad=None):
    return _FusedNoisyConv.apply(x, wq, w_raw, bias, stride, padding,
                                 sigma_mode, factor, want_telemetry,
                                 telemetry_out, current, power_denom, x_pad)


# ---- noisy conv fused with its 2x2 max-pool (small-C image convs) ---------


def conv_pool_eligible(x, w, stride=1, padding=0):
    """Whether fused_noisy_conv2d_pool runs the single-kernel conv+pool pair:
    native 16-bit tensors, stride 1, pad 0, R*S*C <= 128, K <= 96, even
    OH/OW with OW % 4 == 0 (the csrc check adds the LDS-size limits)."""
    if _os.environ.get("NOISYNET_NO_CONV1_POOL"):
        return False
    if not use_native(x, w) or stride != 1 or padding != 0:
        return False
    if x.dtype != w.dtype or x.dim() != 4:
        return False
    return bool(ext().conv_pool_eligible(
        x.shape[1], x.shape[2], x.shape[3], w.shape[0], w.shape[2],
        w.shape[3], x.element_size()))


class _FusedNoisyConvPool(torch.autograd.Function):
    """maxpool2x2(fused noisy conv) as ONE kernel each way.

    Forward gathers the conv's im2col rows from the NHWC input in-kernel
    and pools in registers: neither the im2col matrix nor the un-pooled
    activation reaches memory, and the result (values and argmax code) is
    bit-identical to ``maxpool2x2(fused_noisy_conv2d(...))`` under the same
    seed. Backward is the weight gradient only (first-layer use: the input
    needs no gradient), computed from the pooled gradient, the code and x.
    Saves x, wq and the code -- not the im2col matrix.
    """

    @staticmethod
    def forward(ctx, x, wq, w_raw, bias, sigma_mode, factor):
        ctx.has_bias = bias is not None
        y, code = ext().conv_pool_fwd_fused(
            _nhwc(x), _nhwc(wq), _nhwc(w_raw),
            bias if bias is not None
            else torch.empty(0, device=x.device, dtype=x.dtype),
            1 if sigma_mode == "abs" else 2,
            _factor_tensor(factor, x.device), _next_seed(x.device))
        ctx.save_for_backward(x, wq, code)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, wq, code = ctx.saved_tensors
        gw = gb = None
        if ctx.needs_input_grad[1]:
            gw = ext().conv_pool_wgrad(_nhwc(g), code, _nhwc(x),
                                       wq.shape[2], wq.shape[3])
        if ctx.has_bias and ctx.needs_input_grad[3]:
            # every pooled gradient lands on exactly one un-pooled cell
            gb = g.sum(dim=(0, 2, 3))
        return None, gw, None, gb, None, None


def fused_noisy_conv2d_pool(x, wq, w_raw, bias, stride, padding, sigma_mode,
                            factor, current=0.0, power_denom=1.0,
                            want_telemetry=False, telemetry_out=None):
    """``maxpool2x2(fused_noisy_conv2d(...))``; one fused kernel pair when
    the layer is eligible (see conv_pool_eligible), the input needs no
    gradient and no telemetry is wanted, else exactly that composition
    (also the CPU/reference path). NOISYNET_NO_CONV1_POOL=1 forces the
    composition."""
    if (not want_telemetry and not x.requires_grad
            and conv_pool_eligible(x, wq, stride, padding)):
        return _FusedNoisyConvPool.apply(x, wq, w_raw, bias, sigma_mode,
                                         factor)
    y = fused_noisy_conv2d(x, wq, w_raw, bias, stride, padding, sigma_mode,
                           factor, current=current, power_denom=power_denom,
                           want_telemetry=want_telemetry,
                           telemetry_out=telemetry_out)
    return maxpool2x2(y)


# ---- sigma-only variants (noise tensor alone; used by the standalone
# add_noise_calculate_power API path where the clean output already exists) --


@torch.no_grad()
def sigma_noise_conv2d(x, w_raw, sigma_mode, factor, stride=1, padding=0,
                       want_sigma_abs=False):
    """Return (noise, mean-per-sample sum of sigma_abs or None).

    noise ~ N(0, sqrt(factor*sigma)); the second value is
    mean_over_batch(sum_over_outputs sigma_abs) -- the quantity the power
    formula needs (hardware_model.py:55-57). Native path runs the conv
    kernel with the y-accumulator disabled (sigma accumulator + in-kernel
    Philox Gaussian only) and returns the sum from the kernel's telemetry
    reduction.
    """
    if use_native(x, w_raw):
        noise, tele = ext().sigma_noise_conv(
            _nhwc(x), _nhwc(w_raw), stride, padding,
            1 if sigma_mode == "abs" else 2, _factor_tensor(factor, x.device),
            _next_seed(x.device), bool(want_sigma_abs))
        sig_mean = tele[0] / x.shape[0] if want_sigma_abs else None
        return noise, sig_mean
    sig = ref.sigma_conv2d(x, w_raw, sigma_mode, stride, padding)
    noise = ref.vmm_noise(sig, factor)
    sig_mean = None
    if want_sigma_abs:
        sig_abs = sig if sigma_mode == "abs" else ref.sigma_conv2d(x, w_raw, "abs", stride, padding)
        sig_mean = sig_abs.sum(dim=(1, 2, 3)).mean()
    return noise, sig_mean


@torch.no_grad()
def sigma_noise_linear(x, w_raw, sigma_mode, factor, want_sigma_abs=False):
    if use_native(x, w_raw):
        noise, tele = ext().sigma_noise_linear(
            x.contiguous(), w_raw.contiguous(),
            1 if sigma_mode == "abs" else 2, _factor_tensor(factor, x.device),
            _next_seed(x.device), bool(want_sigma_abs))
        sig_mean = tele[0] / x.shape[0] if want_sigma_abs else None
        return noise, sig_mean
    sig = ref.sigma_linear(x, w_raw, sigma_mode)
    noise = ref.vmm_noise(sig, factor)
    sig_mean = None
    if want_sigma_abs:
        sig_abs = sig if sigma_mode == "abs" else ref.sigma_linear(x, w_raw, "abs")
        sig_mean = sig_abs.sum(dim=1).mean()
    return noise, sig_mean


# ---- Linear twins ---------------------------------------------------------


def _linear_fwd_raw(x, w, bias):
    # Plain (un-fused) linear IS a library GEMM: hipBLASLt via F.linear
    # beats our MFMA kernel on the fc shapes (0.023 vs 0.172 ms for
    # 2048x3000 @ 390x3000 bf16 on MI355X). The custom kernel stays for
    # the FUSED noisy path (linear_fwd_fused) where sigma+noise ride the
    # same tiles, and is still exercised directly in tests/test_ops_gpu.
    return F.linear(x, w, bias)


class LinearFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return _linear_fwd_raw(x, w, bias)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = LinearDgrad.apply(g, w)
        if ctx.needs_input_grad[1]:
            gw = LinearWgrad.apply(g, x)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(dim=0)
        return gx, gw, gb


class LinearDgrad(torch.autograd.Function):
    """dx = g @ W  (g:[B,O], W:[O,I] -> dx:[B,I])."""

    @staticmethod
    def forward(ctx, g, w):
        ctx.save_for_backward(g, w)
        return g.matmul(w)  # plain GEMM -> hipBLASLt

    @staticmethod
    def backward(ctx, gg):
        g, w = ctx.saved_tensors
        d_g = d_w = None
        if ctx.needs_input_grad[0]:
            d_g = LinearFwd.apply(gg, w, None)
        if ctx.needs_input_grad[1]:
            d_w = LinearWgrad.apply(g, gg)
        return d_g, d_w


class LinearWgrad(torch.autograd.Function):
    """dW = g^T @ x  (g:[B,O], x:[B,I] -> dW:[O,I])."""

    @staticmethod
    def forward(ctx, g, x):
        ctx.save_for_backward(g, x)
        return g.t().matmul(x)  # plain GEMM -> hipBLASLt

    @staticmethod
    def backward(ctx, gw):
        g, x = ctx.saved_tensors
        d_g = d_x = None
        if ctx.needs_input_grad[0]:
            # d/dg of (g^T x) contracted with gw: x @ gw^T = linear(x, gw)
            d_g = LinearFwd.apply(x, gw, None)
        if ctx.needs_input_grad[1]:
            d_x = LinearDgrad.apply(g, gw)
        return d_g, d_x


def linear(x, w, bias=None):
    return LinearFwd.apply(x, w, bias)


class _FusedNoisyLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wq, w_raw, bias, sigma_mode, factor,
                want_telemetry, telemetry_out, current, power_denom):
        ctx.save_for_backward(x, wq)
        ctx.has_bias = bias is not None
        if use_native(x, wq):
            y, tele = ext().linear_fwd_fused(
                x.contiguous(), wq.contiguous(), w_raw.contiguous(),
                bias if bias is not None else torch.empty(0, device=x.device, dtype=x.dtype),
                1 if sigma_mode == "abs" else 2,
                _factor_tensor(factor, x.device),
                _next_seed(x.device), bool(want_telemetry))
            if want_telemetry:
                sum_sigma_abs = tele[0] / x.shape[0]
                sum_abs_noise = tele[1] / y.numel()
                max_y = tele[2]
        else:
            y = F.linear(x, wq, bias)
            with torch.no_grad():
                sig = ref.sigma_linear(x.detach(), w_raw, sigma_mode)
                noise = ref.vmm_noise(sig, factor)
                if want_telemetry:
                    sig_abs = sig if sigma_mode == "abs" else ref.sigma_linear(x.detach(), w_raw, "abs")
                    sum_sigma_abs = sig_abs.sum(dim=1).mean()
                    sum_abs_noise = noise.abs().mean()
                    max_y = y.detach().max()
            y = y + noise
        if want_telemetry and telemetry_out is not None:
            with torch.no_grad():
                telemetry_out.power = 1.2e-6 * current * sum_sigma_abs / power_denom
                telemetry_out.nsr = sum_abs_noise / max_y
                telemetry_out.input_sparsity = (x.detach() > 0).sum() / x.numel()
        return y

    @staticmethod
    def backward(ctx, g):
        x, wq = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = LinearDgrad.apply(g, wq)
        if ctx.needs_input_grad[1]:
            gw = LinearWgrad.apply(g, x)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = g.sum(dim=0)
        return (gx, gw, None, gb) + (None,) * 6


def fused_noisy_linear(x, wq, w_raw, bias, sigma_mode, factor, current=0.0,
                       power_denom=1.0, want_telemetry=False, telemetry_out=None):
    return _FusedNoisyLinear.apply(x, wq, w_raw, bias, sigma_mode, factor,
                                   want_telemetry, telemetry_out, current,
                                   power_denom)


# ---------------------------------------------------------------------------
# Tiled crossbars: the contraction is cut into blocks of xbar_rows rows, each
# with its own current noise and its own ADC; the digital side adds the blocks
# ---------------------------------------------------------------------------


class XbarTelemetry(NoiseTelemetry):
    """NoiseTelemetry of a tiled-crossbar call plus the ADC statistics:
    ``adc_clip_share`` (share of block partials beyond the ADC range) and
    ``partial_absmax`` (max |v_b| over every block partial -- the value to
    pick ``adc_max`` from). power / nsr stay None when the noise is off.

    With differential columns both figures are per COLUMN partial: the share
    is over the 2 * nblocks * M * K column values v+ / v- (beyond the top code
    or below zero), ``partial_absmax`` is the max |v+-|, and nsr uses the
    digital difference of the two columns' noises.

    With bit-serial inputs (``dac_bits`` > 0, J slices) both figures are per
    SLICE partial: the share is over the J * nblocks * M * K values v_bj and
    ``partial_absmax`` is the max |v_bj| -- the number to size the per-slice
    ``adc_max`` from, much smaller than the unsliced one. power is what the
    unsliced op reports for on-grid inputs; nsr uses the shift-added noise.

    With bit-sliced weights (``cell_bits`` > 0, T slices) both figures are per
    cell SLICE partial: the share is over the T * nblocks * M * K unipolar
    column values v_bt (beyond the top code or below zero) and
    ``partial_absmax`` is the max |v_bt|, the number to size the per-slice
    ``adc_max`` from. power is computed from the current the offset-binary
    cells draw (sum p_bt, not shift-weighted), which is higher than the
    signed one-cell model's; nsr uses the shift-added noise."""

    __slots__ = ("adc_clip_share", "partial_absmax")

    def __init__(self, power=None, nsr=None, input_sparsity=None,
                 adc_clip_share=None, partial_absmax=None):
        super().__init__(power, nsr, input_sparsity)
        self.adc_clip_share = adc_clip_share
        self.partial_absmax = partial_absmax


_XBAR_MODE = {None: 0, "abs": 1, "abs2": 2}


def _check_cells(cells, wq, w_bits, cell_bits):
    slices = -(-int(w_bits) // int(cell_bits))
    want = (slices, wq.shape[0], wq[0].numel())
    if not isinstance(cells, torch.Tensor) or tuple(cells.shape) != want:
        raise ValueError(
            "cells must be the tensor G of xbar_program_cells with the shape "
            "%r (slices, output columns, crossbar rows), got %r"
            % (want, getattr(cells, "shape", cells)))


def xbar_program_cells(wq, w_bits, cell_bits, w_step, w_min, sigma=0.0,
                       p_stuck_off=0.0, p_stuck_on=0.0, seed=None):
    """Program a layer's weight codes onto imperfect cells, once: returns the
    conductances G[T, K, n] (digit units, the dtype of ``wq``) that
    xbar_noisy_conv2d / xbar_noisy_linear read through ``cells=``.

    ``wq`` is a conv filter [K, C, R, S] or a linear weight [K, n] on the
    grid w = ``w_min`` + code * ``w_step`` (``w_bits`` = B bits), n = R*S*C in
    the crossbar-row order (r, s, c), c fastest; T = ceil(B / E) slices of
    ``cell_bits`` = E bit cells. For slice t, output column k and row i
        code   = clamp(rint((f32(wq) - w_min) * (1/w_step)), 0, 2^B - 1)
        d_t    = (code >> t*E) & (2^E - 1)
        (u, z) = one Philox4x32 draw, key = chip seed,
                 counter = (t*K + k)*n + i; u uniform on [0, 1) from word 0,
                 z ~ N(0, 1) by Box-Muller on words 2 and 3
        d'_t   = 0         if u < p_stuck_off   (stuck at the high-resistance
                                                 state)
               = 2^E - 1   else if u < p_stuck_off + p_stuck_on  (stuck on:
                                                 the top level of the cell)
               = d_t       otherwise
        G_t    = round_to_dtype(max(d'_t * (1 + sigma * z), 0))
    in fp32 with the one rounding. The variation is multiplicative and
    Gaussian, clamped at zero: an off cell stays off, and a stuck-on cell is
    still an analog device and varies like any other. Log-normal variation
    and additive HRS leakage are not modelled.

    ``seed`` None draws a fresh chip: the next seed of the global stream,
    sent through the graph seed so that a captured step programs a new chip
    on every replay. An int is one fixed chip, in eager mode and under
    capture alike. One HIP launch on the GPU (for the 16-bit dtypes the rows
    of the result sit at a pitch padded to 8 elements; the [T, K, n] tensor
    returned is that view and the fused op reads it in place); CPU tensors
    use the reference twin, which draws the same distribution from a
    torch.Generator."""
    ref.xbar_check_cell_args(w_bits, cell_bits, w_step, w_min, "abs", 0)
    ref.xbar_check_program_args(sigma, p_stuck_off, p_stuck_on)
    wq = wq.detach()
    cell = ref.xbar_cell_params(w_step, w_min, wq.device)
    if use_native(wq):
        fresh = seed is None
        s = _next_seed(wq.device) if fresh else int(seed)
        w = _nhwc(wq) if wq.dim() == 4 else wq.contiguous()
        return ext().xbar_program_cells(w, int(w_bits), int(cell_bits), cell,
                                        float(sigma), float(p_stuck_off),
                                        float(p_stuck_on), s, fresh)
    gen = None
    if seed is not None:
        gen = torch.Generator(device=wq.device).manual_seed(int(seed))
    return ref.xbar_program_cells(wq, w_bits, cell_bits, cell, sigma,
                                  p_stuck_off, p_stuck_on, gen)


def _xbar_forward(x2_or_x, is_conv, wq, w_raw, bias, stride, padding,
                  sigma_mode, factor, xbar_rows, adc_bits, adc_max,
                  want_telemetry, differential=False, in_bits=0, dac_bits=0,
                  x_step=None, w_bits=0, cell_bits=0, w_step=None, w_min=None,
                  cells=None):
    """Shared forward of the two xbar Functions. Returns (y, tele) with tele a
    dict of 0-dim tensors (or None): sigma_abs, abs_noise, max_y, clipped,
    n_partials, partial_absmax -- sums over the whole call. ``differential``
    runs W+ / W- columns with unipolar ADCs (two partials per block);
    ``dac_bits`` > 0 streams the input in J slices (J partials per block);
    ``cell_bits`` > 0 spreads the weight code over T columns with unipolar
    ADCs (T partials per block); ``cells`` then reads the programmed
    conductances G[T, K, n] in place of the digits."""
    x = x2_or_x
    differential = bool(differential)
    adc = ref.xbar_adc_params(adc_bits, adc_max, x.device,
                              unipolar=differential or bool(cell_bits))
    n_rows = wq[0].numel()
    nblocks = -(-n_rows // int(xbar_rows))
    dac, serial, slices = None, (), 1
    cell = None
    if cell_bits:
        slices = -(-int(w_bits) // int(cell_bits))
        cell = ref.xbar_cell_params(w_step, w_min, x.device)
        serial = (int(w_bits), int(cell_bits), cell)
        fwd_conv, fwd_linear = "xbar_cells_fwd_conv", "xbar_cells_fwd_linear"
        if cells is not None:
            fwd_conv, fwd_linear = "xbar_prog_fwd_conv", "xbar_prog_fwd_linear"
    elif dac_bits:
        slices = -(-int(in_bits) // int(dac_bits))
        dac = ref.xbar_dac_params(x_step, x.device)
        serial = (int(in_bits), int(dac_bits), dac)
        fwd_conv, fwd_linear = "xbar_serial_fwd_conv", "xbar_serial_fwd_linear"
    elif differential:
        fwd_conv, fwd_linear = "xbar_diff_fwd_conv", "xbar_diff_fwd_linear"
    else:
        fwd_conv, fwd_linear = "xbar_fwd_conv", "xbar_fwd_linear"
    if use_native(x, wq):
        empty = torch.empty(0, device=x.device, dtype=x.dtype)
        empty_f = torch.empty(0, device=x.device, dtype=torch.float32)
        common = (_XBAR_MODE[sigma_mode],
                  _factor_tensor(factor, x.device) if sigma_mode is not None
                  else torch.zeros(1, device=x.device, dtype=torch.float32),
                  int(xbar_rows), int(adc_bits),
                  adc if adc is not None else empty_f) + serial + (
                  _next_seed(x.device), bool(want_telemetry))
        wr = w_raw if sigma_mode is not None else wq
        if cell_bits:       # the conductances are the digits: no w_raw
            prog = () if cells is None else (cells.detach(),)
            if is_conv:
                y, t = getattr(ext(), fwd_conv)(
                    _nhwc(x), _nhwc(wq), *prog,
                    bias if bias is not None else empty,
                    stride, padding, *common)
            else:
                y, t = getattr(ext(), fwd_linear)(
                    x.contiguous(), wq.contiguous(), *prog,
                    bias if bias is not None else empty, *common)
        elif is_conv:
            y, t = getattr(ext(), fwd_conv)(
                _nhwc(x), _nhwc(wq), _nhwc(wr),
                bias if bias is not None else empty, stride, padding, *common)
        else:
            y, t = getattr(ext(), fwd_linear)(
                x.contiguous(), wq.contiguous(), wr.contiguous(),
                bias if bias is not None else empty, *common)
        tele = None
        if want_telemetry:
            tele = dict(sigma_abs=t[0], abs_noise=t[1], max_y=t[2],
                        clipped=t[3],
                        n_partials=(2 if differential else slices) * nblocks
                        * y.numel(),
                        partial_absmax=t[4])
        return y, tele
    tele = {} if want_telemetry else None
    with torch.no_grad():
        xd = x.detach()
        if is_conv:
            R, S = wq.shape[2], wq.shape[3]
            xm = ref.xbar_conv_rows(xd.float(), R, S, stride, padding)
        else:
            xm = xd
        ym = ref.xbar_vmm(
            xm, ref.xbar_weight_rows(wq.detach()),
            ref.xbar_weight_rows(w_raw.detach())
            if sigma_mode is not None and not cell_bits else None,
            bias.detach() if bias is not None else None, sigma_mode, factor,
            int(xbar_rows), adc_bits, adc, stats=tele,
            differential=differential, dac=dac, in_bits=int(in_bits),
            dac_bits=int(dac_bits), cell=cell, w_bits=int(w_bits),
            cell_bits=int(cell_bits),
            **({} if cells is None else dict(cells=cells.detach())))
        if is_conv:
            N, K = x.shape[0], wq.shape[0]
            oh = (x.shape[2] + 2 * padding - R) // stride + 1
            ow = (x.shape[3] + 2 * padding - S) // stride + 1
            ym = ym.view(N, oh, ow, K).permute(0, 3, 1, 2)
        y = ym.to(x.dtype)
        if is_conv:
            y = y.contiguous(memory_format=torch.channels_last) if x.is_cuda \
                else y.contiguous()
    return y, tele


def _xbar_publish(telemetry_out, tele, x, y, sigma_mode, current,
                  power_denom):
    with torch.no_grad():
        if sigma_mode is not None:
            telemetry_out.power = 1.2e-6 * current \
                * (tele["sigma_abs"] / x.shape[0]) / power_denom
            telemetry_out.nsr = (tele["abs_noise"] / y.numel()) / tele["max_y"]
        telemetry_out.input_sparsity = (x.detach() > 0).sum() / x.numel()
        telemetry_out.adc_clip_share = tele["clipped"] / tele["n_partials"]
        telemetry_out.partial_absmax = tele["partial_absmax"]


class _XbarNoisyConv(torch.autograd.Function):
    """Tiled-crossbar conv: per-block noise + ADC fused into one MFMA pass
    (xbar_fwd_kernel, csrc/xbar_fwd.hip). Backward is the identity
    straight-through over the noise and the ADC: exactly the gradients of the
    unblocked conv with wq. A clipped STE would need per-block saturation
    masks and is not built. ``differential`` selects xbar_diff_fwd_kernel
    (W+ / W- columns, unipolar ADCs), ``dac_bits`` > 0 xbar_serial_fwd_kernel
    (bit-serial inputs, csrc/xbar_serial.hip), ``cell_bits`` > 0
    xbar_cells_fwd_kernel (bit-sliced weights, csrc/xbar_cells.hip; with
    ``cells`` its programmed path, which reads the conductances G of
    xbar_program_cells in place of the digits); the backward is the same."""

    @staticmethod
    def forward(ctx, x, wq, w_raw, bias, stride, padding, sigma_mode, factor,
                xbar_rows, adc_bits, adc_max, want_telemetry, telemetry_out,
                current, power_denom, differential=False, in_bits=0,
                dac_bits=0, x_step=None, w_bits=0, cell_bits=0, w_step=None,
                w_min=None, cells=None):
        ctx.stride, ctx.padding = stride, padding
        ctx.has_bias = bias is not None
        y, tele = _xbar_forward(x, True, wq, w_raw, bias, stride, padding,
                                sigma_mode, factor, xbar_rows, adc_bits,
                                adc_max, want_telemetry, differential,
                                in_bits, dac_bits, x_step, w_bits, cell_bits,
                                w_step, w_min, cells)
        if want_telemetry and telemetry_out is not None:
            _xbar_publish(telemetry_out, tele, x, y, sigma_mode, current,
                          power_denom)
        ctx.save_for_backward(x, wq)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wq = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ConvDgrad.apply(g, wq, ctx.stride, ctx.padding, x.shape)
        if ctx.needs_input_grad[1]:
            gw = ConvWgrad.apply(g, x, ctx.stride, ctx.padding, wq.shape, None)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = g.sum(dim=(0, 2, 3))
        return (gx, gw, None, gb) + (None,) * 20


class _XbarNoisyLinear(torch.autograd.Function):
    """Linear twin of _XbarNoisyConv (same kernel, R = S = 1)."""

    @staticmethod
    def forward(ctx, x, wq, w_raw, bias, sigma_mode, factor, xbar_rows,
                adc_bits, adc_max, want_telemetry, telemetry_out, current,
                power_denom, differential=False, in_bits=0, dac_bits=0,
                x_step=None, w_bits=0, cell_bits=0, w_step=None, w_min=None,
                cells=None):
        ctx.has_bias = bias is not None
        y, tele = _xbar_forward(x, False, wq, w_raw, bias, 1, 0, sigma_mode,
                                factor, xbar_rows, adc_bits, adc_max,
                                want_telemetry, differential, in_bits,
                                dac_bits, x_step, w_bits, cell_bits, w_step,
                                w_min, cells)
        if want_telemetry and telemetry_out is not None:
            _xbar_publish(telemetry_out, tele, x, y, sigma_mode, current,
                          power_denom)
        ctx.save_for_backward(x, wq)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wq = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = LinearDgrad.apply(g, wq)
        if ctx.needs_input_grad[1]:
            gw = LinearWgrad.apply(g, x)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            gb = g.sum(dim=0)
        return (gx, gw, None, gb) + (None,) * 18


def xbar_noisy_conv2d(x, wq, w_raw, bias, stride, padding, sigma_mode, factor,
                      xbar_rows, adc_bits, adc_max, current=0.0,
                      power_denom=1.0, want_telemetry=False,
                      telemetry_out=None, differential=False, in_bits=0,
                      dac_bits=0, x_step=None, w_bits=0, cell_bits=0,
                      w_step=None, w_min=None, cells=None):
    """Noisy conv on tiled crossbars.

    The contraction index is the filter's memory order (r, s, c), c fastest;
    padding positions contribute zero. Block b is rows [b*xbar_rows,
    min((b+1)*xbar_rows, R*S*C)); ``xbar_rows`` is a positive multiple of 32
    and the last block may be short. Per block, in fp32,
        p_b = sum x*wq          s_b = max(sum x*f(|w_raw|), 0)
        v_b = p_b + eps_b * sqrt(factor * s_b)       eps_b ~ N(0,1) per block
        q_b = step * clamp(rint(v_b * (1/step)), -Qm, Qm)
    with Qm = 2^(adc_bits-1) - 1, step = adc_max / Qm, and
    out = sum_b q_b + bias, rounded once to the dtype. ``sigma_mode`` None
    switches the noise off (v_b = p_b), ``adc_bits`` 0 the ADC (q_b = v_b);
    one of the two must be on. ``adc_max`` is a number or a tensor (then it
    must be positive; it is not read back to check).

    Backward is the identity straight-through over noise and ADC: the
    gradients are exactly those of conv2d(x, wq, bias). A clipped STE (zero
    gradient through saturated blocks) would need per-block saturation masks
    and is out of scope.

    ``telemetry_out`` (an XbarTelemetry) receives power / nsr / sparsity as
    fused_noisy_conv2d does, plus adc_clip_share and partial_absmax.

    ``differential=True`` puts the positive and the negative part of the
    weights on two columns, each with its own noise draw and its own unipolar
    ADC, subtracted digitally. Per block, in fp32,
        wq+ = max(wq, 0)    wq- = max(-wq, 0)       (by the sign of wq)
        f+- = f(|w_raw|) where w_raw > 0 / < 0, else 0
        p+- = sum x*wq+-    s+- = max(sum x*f+-, 0)
        v+- = p+- + eps+- * sqrt(factor * s+-)      eps+, eps- independent
        q+- = step * clamp(rint(v+- * (1/step)), 0, Qu)
    with Qu = 2^adc_bits - 1, step = adc_max / Qu, and
    out = sum_b (q+ - q-) + bias. A column value that rounds below 0 clamps to
    0 and counts as clipped. The op does not inspect the sign of x; the mode
    is meant for non-negative activations (post-ReLU, or images in [0, 1]),
    where each column carries a non-negative current. The telemetry's ADC
    figures are then per column partial (2 * nblocks per output). The backward
    is unchanged.

    ``dac_bits`` = D > 0 streams the activation bit-serially: x is an
    ``in_bits`` = B bit code on the grid ``x_step`` (the activation LSB, a
    positive number or 1-element tensor) and reaches the rows D bits per
    cycle, J = ceil(B / D) <= 4 slices. B is 1..8, at most 7 for bf16 (which
    does not carry every 8-bit code). Per block b and slice j, in fp32,
        code = clamp(rint(x * (1/x_step)), 0, 2^B - 1)
        d_j  = (code >> j*D) & (2^D - 1)       (the top slice may be narrower)
        p_bj = x_step * sum d_j*wq     s_bj = max(x_step * sum d_j*f(|w_raw|), 0)
        v_bj = p_bj + eps_bj * sqrt(factor * s_bj)   own draw per (b, j)
        q_bj = step * clamp(rint(v_bj * (1/step)), -Qm, Qm)
    and out = sum_b sum_j 2^(jD) q_bj + bias (b ascending, j ascending inside
    b), rounded once. The op RE-QUANTISES its input: negative values clamp to
    code 0 and off-grid values round to the grid, so feed it the output of
    the activation quantiser with that quantiser's step. ``factor`` is the
    one of the unsliced layer -- the model is "same cell current per unit
    input, one conversion per slice" -- so the noise drawn in slice j is
    multiplied by 2^(jD) in the shift-add and the output noise variance is
    factor * sum_b sum_j 4^(jD) s_bj, larger than the unsliced
    factor * sum_b s_b. ``adc_max`` is the range of ONE slice conversion; the
    partials are much smaller than unsliced ones (read ``partial_absmax``).
    The telemetry's ADC figures are per slice partial (J * nblocks per
    output). ``dac_bits`` = 0 is the op without slicing. Differential columns
    with bit-serial inputs are not built. The backward is unchanged.

    ``cell_bits`` = E in 1..4 slices the WEIGHTS: a cell holds E bits, so the
    ``w_bits`` = B bit (1..8) offset-binary code of a weight on the grid
    w = ``w_min`` + code * ``w_step`` (the weight quantiser's grid; numbers or
    1-element tensors) is spread over T = ceil(B / E) <= 4 columns, each with
    its own current, noise draw and UNIPOLAR ADC conversion; the digital side
    shift-adds the columns and adds the offset. Per block b and slice t, in
    fp32,
        code = clamp(rint((wq - w_min) * (1/w_step)), 0, 2^B - 1)
        d_t  = (code >> t*E) & (2^E - 1)      cell conductance g_t = w_step*d_t
        p_bt = w_step * sum x*d_t
        s_bt = max(sum x*f(g_t), 0)           f = g (abs), g^2 + g (abs2)
        v_bt = p_bt + eps_bt * sqrt(factor * s_bt)   own draw per (b, t)
        q_bt = step * clamp(rint(v_bt * (1/step)), 0, Qu)
        X_b  = sum x                          (digital, exact)
    with Qu = 2^adc_bits - 1, step = adc_max / Qu, and
    out = sum_b (sum_t 2^(tE) q_bt + w_min * X_b) + bias, rounded once. The
    weights are recovered from ``wq`` as codes, so with noise and ADC off the
    op would compute x @ W_grid^T with the exact grid weights, not with the
    dtype-rounded ``wq``; ``w_raw`` is not used -- the noise comes from the
    cells, whose conductances are the digits. ``factor`` stays that of the
    unsliced layer, so the output noise variance is
    factor * sum_b sum_t 4^(tE) s_bt. Offset-binary cells carry current even
    for a zero weight (code -w_min/w_step), so noise and power are higher than
    the signed one-cell model's. ``adc_max`` is the range [0, adc_max] of ONE
    column conversion (read ``partial_absmax``); the telemetry's ADC figures
    are per slice partial (T * nblocks per output) and ``power`` is computed
    from the current the cells draw, sum p_bt, not shift-weighted. Not
    combinable with ``differential`` or ``dac_bits``. ``cell_bits`` = 0 is the
    op with one analog cell per weight. The backward is unchanged.

    ``cells`` = G[T, K, R*S*C] (needs ``cell_bits`` > 0) runs the bit-sliced
    op on PROGRAMMED cells: the tensor xbar_program_cells wrote (conductance
    variation, stuck-at cells; digit units, the dtype of x) stands in for the
    ideal digits,
        p_bt = w_step * sum x*G_t
        s_bt = max(p_bt, 0)                                           (abs)
             = max(w_step^2 * sum x*round_to_dtype(G_t^2) + p_bt, 0)  (abs2)
    and everything from v_bt on, the exact digital offset w_min * X_b
    included, is the model above. ``wq`` then gives the geometry and the
    gradients only: the backward stays that of conv2d(x, wq, bias).
    ``cells`` = None is the ideal-digit op exactly.
    """
    if isinstance(stride, (tuple, list)):
        stride = stride[0]
    if isinstance(padding, (tuple, list)):
        padding = padding[0]
    cells_args = ()
    if cell_bits:
        ref.xbar_check_cell_args(w_bits, cell_bits, w_step, w_min, sigma_mode,
                                 adc_bits, differential, dac_bits)
        cells_args = (w_bits, cell_bits, w_step, w_min)
    elif dac_bits:
        ref.xbar_check_serial_args(in_bits, dac_bits, x_step, x.dtype,
                                   sigma_mode, adc_bits, differential)
    elif cells is not None:
        raise ValueError("cells (programmed conductances) needs cell_bits > 0")
    ref.xbar_check_args(sigma_mode, xbar_rows, adc_bits, adc_max)
    if cells is not None:
        _check_cells(cells, wq, w_bits, cell_bits)
        cells_args = cells_args + (cells,)
    return _XbarNoisyConv.apply(x, wq, w_raw, bias, stride, padding,
                                sigma_mode, factor, xbar_rows, adc_bits,
                                adc_max, want_telemetry, telemetry_out,
                                current, power_denom, bool(differential),
                                in_bits, dac_bits, x_step, *cells_args)


def xbar_noisy_linear(x, wq, w_raw, bias, sigma_mode, factor, xbar_rows,
                      adc_bits, adc_max, current=0.0, power_denom=1.0,
                      want_telemetry=False, telemetry_out=None,
                      differential=False, in_bits=0, dac_bits=0, x_step=None,
                      w_bits=0, cell_bits=0, w_step=None, w_min=None,
                      cells=None):
    """Noisy linear layer on tiled crossbars: xbar_noisy_conv2d with the input
    index as the crossbar row. Same straight-through backward (the gradients
    of F.linear(x, wq, bias)); a clipped STE is out of scope.
    ``differential=True`` selects the W+ / W- columns with unipolar ADCs
    described there (meant for non-negative activations); ``dac_bits`` > 0
    the bit-serial inputs described there (``in_bits``, ``x_step``),
    ``cell_bits`` > 0 the bit-sliced weights described there (``w_bits``,
    ``w_step``, ``w_min``), ``cells`` = G[T, K, n] the programmed cells
    described there."""
    cells_args = ()
    if cell_bits:
        ref.xbar_check_cell_args(w_bits, cell_bits, w_step, w_min, sigma_mode,
                                 adc_bits, differential, dac_bits)
        cells_args = (w_bits, cell_bits, w_step, w_min)
    elif dac_bits:
        ref.xbar_check_serial_args(in_bits, dac_bits, x_step, x.dtype,
                                   sigma_mode, adc_bits, differential)
    elif cells is not None:
        raise ValueError("cells (programmed conductances) needs cell_bits > 0")
    ref.xbar_check_args(sigma_mode, xbar_rows, adc_bits, adc_max)
    if cells is not None:
        _check_cells(cells, wq, w_bits, cell_bits)
        cells_args = cells_args + (cells,)
    return _XbarNoisyLinear.apply(x, wq, w_raw, bias, sigma_mode, factor,
                                  xbar_rows, adc_bits, adc_max,
                                  want_telemetry, telemetry_out, current,
                                  power_denom, bool(differential), in_bits,
                                  dac_bits, x_step, *cells_args)


# ---------------------------------------------------------------------------
# Simplified noise modes (uniform_ind / uniform_dep / normal_ind / normal_dep)
# hardware_model.py:24-41 -- train-time or --noise_test perturbations.
# ---------------------------------------------------------------------------


def simple_noise(output, mode, a):
    """Returns the noise tensor (detached). Modes per hardware_model.py:24-41."""
    with torch.no_grad():
        out = output.detach()
        if mode == "uniform_ind":
            amp = a * out.abs().max()
            return torch.empty_like(out).uniform_(-1, 1) * amp
        if mode == "uniform_dep":
            lo = torch.full_like(out, a)
            hi = torch.full_like(out, 1.0 / a)
            return lo + (hi - lo) * torch.rand_like(out)
        if mode == "normal_ind":
            s = a * out.abs().max()
            return torch.randn_like(out) * s
        if mode == "normal_dep":
            return torch.randn_like(out) * (a * out)  # signed scale, as reference
        raise ValueError(mode)


# ---------------------------------------------------------------------------
# Elementwise weight perturbation (AddNoise STE)
# ---------------------------------------------------------------------------


class MultUniformNoise(torch.autograd.Function):
    """out = w + w*U(-a,a); identity STE backward (hardware_model.py:291-307)."""

    @staticmethod
    def forward(ctx, w, a):
        if use_native(w):
            return ext().mult_uniform_noise(w, float(a), _next_seed(w.device))
        return ref.mult_uniform_noise(w, a)

    @staticmethod
    def backward(ctx, g):
        return g, None


def add_weight_noise(w, a):
    return MultUniformNoise.apply(w, a)


# ---------------------------------------------------------------------------
# Fused BatchNorm + ReLU + clip
# ---------------------------------------------------------------------------


def _act_mask(y, relu, act_max):
    """Activation mask re-derived from the stored output y: dy/dz = 1 where
    0 < y (< act_max if clipped). A saturated element is stored as act_max
    ROUNDED to y's dtype (0.7 is 0.69921875 in bf16), so y is compared with
    that stored value: against the f32 threshold a threshold that rounds
    down would never mask. Same rule as the HIP kernels (stored_act_max in
    csrc/common.h)."""
    mask = torch.ones_like(y, dtype=torch.bool)
    if relu:
        mask &= y > 0
    if act_max > 0:
        thr = torch.tensor(float(act_max), dtype=torch.float32).to(y.dtype)
        mask &= y < thr
    return mask


class BnAct(torch.autograd.Function):
    """BN (train: batch stats; eval: running stats) fused with ReLU and an
    optional upper clip. Backward folds the activation mask into the BN
    gradient. Native path: csrc/bn_act.hip (per-channel partials + one fused
    normalize/act pass).

    ``sync=True`` is the fused SyncBN (main.py:786-796 equivalent): the
    per-rank (mean, E[x^2]) pairs are combined with ONE RCCL all-reduce
    before normalization, and the backward's per-channel sums are likewise
    all-reduced before the apply pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training,
                momentum, eps, relu, act_max, sync=False):
        import torch.distributed as dist
        ws = dist.get_world_size() if (sync and dist.is_initialized()) else 1
        ctx.sync_ws = ws if training else 1
        if (training and ws == 1 and use_native(x)
                and (running_mean is None
                     or running_mean.dtype == torch.float32)):
            # fused single-rank path: stats + invstd + running update in
            # two kernels (the eager chain was ~8 tiny launches per layer)
            xc = _nhwc(x) if x.dim() == 4 else x.contiguous()
            empty = torch.empty(0, device=x.device, dtype=torch.float32)
            mean, invstd = ext().bn_stats_finalize(
                xc,
                running_mean if running_mean is not None else empty,
                running_var if running_var is not None else empty,
                float(momentum), float(eps))
            if use_native(x):
                y = ext().bn_act_fwd(xc, mean, invstd,
                                     weight.float().contiguous(),
                                     bias.float().contiguous(),
                                     bool(relu), float(act_max))
            ctx.save_for_backward(x, weight, mean, invstd, y)
            ctx.training = training
            ctx.relu, ctx.act_max = relu, act_max
            return y
        if training:
            if use_native(x):
                mean, var = ext().bn_stats(_nhwc(x) if x.dim() == 4 else x.contiguous())
            else:
                # f32 statistics whatever the storage dtype, as the kernel
                mean, var = ref.bn_stats(x.float())
            if ws > 1:
                stats = torch.stack([mean, var + mean * mean])
                dist.all_reduce(stats)
                stats /= ws
                mean = stats[0]
                var = (stats[1] - mean * mean).clamp_min(0)
            if running_mean is not None:
                with torch.no_grad():
                    n = x.numel() / x.shape[1] * ws
                    unbiased = var * (n / max(n - 1.0, 1.0))
                    running_mean.mul_(1 - momentum).add_(momentum * mean.to(running_mean.dtype))
                    running_var.mul_(1 - momentum).add_(momentum * unbiased.to(running_var.dtype))
        else:
            mean = running_mean
            var = running_var
        mean = mean.float()
        invstd = (var.float() + eps).rsqrt()
        if use_native(x):
            y = ext().bn_act_fwd(_nhwc(x) if x.dim() == 4 else x.contiguous(),
                                 mean.contiguous(), invstd.contiguous(),
                                 weight.float().contiguous(),
                                 bias.float().contiguous(),
                                 bool(relu), float(act_max))
        else:
            y = ref.bn_act_forward(x.float(), weight.float(), bias.float(),
                                   mean, invstd, act_max, relu).to(x.dtype)
        ctx.save_for_backward(x, weight, mean, invstd, y)
        ctx.training = training
        ctx.relu, ctx.act_max = relu, act_max
        return y

    @staticmethod
    def backward(ctx, g):
        import torch.distributed as dist
        x, weight, mean, invstd, y = ctx.saved_tensors
        ws = getattr(ctx, 'sync_ws', 1)
        if use_native(x):
            gc = _nhwc(g) if g.dim() == 4 else g.contiguous()
            xc = _nhwc(x) if x.dim() == 4 else x.contiguous()
            yc = _nhwc(y) if y.dim() == 4 else y.contiguous()
            if ws > 1:
                sum_g_loc, sum_gx_loc = ext().bn_act_bwd_reduce(
                    gc, xc, yc, mean.contiguous(), invstd.contiguous(),
                    bool(ctx.relu), float(ctx.act_max))
                pair = torch.stack([sum_g_loc, sum_gx_loc])
                dist.all_reduce(pair)
                sum_g, sum_gx = pair[0].contiguous(), pair[1].contiguous()
                count = x.numel() / x.shape[1] * ws
                gx = ext().bn_act_bwd_apply(
                    gc, xc, yc, mean.contiguous(), invstd.contiguous(),
                    weight.float().contiguous(), sum_g, sum_gx, float(count),
                    bool(ctx.training), bool(ctx.relu), float(ctx.act_max))
                # gamma/beta grads stay LOCAL sums: the data-parallel bucket
                # all-reduce averages them like torch SyncBatchNorm expects
                return (gx, sum_gx_loc.to(weight.dtype),
                        sum_g_loc.to(weight.dtype)) + (None,) * 8
            gx, g_gamma, g_beta = ext().bn_act_bwd(
                gc, xc, yc, mean.contiguous(), invstd.contiguous(),
                weight.float().contiguous(), bool(ctx.training),
                bool(ctx.relu), float(ctx.act_max))
            return (gx, g_gamma.to(weight.dtype),
                    g_beta.to(weight.dtype)) + (None,) * 8
        shape = (1, -1, 1, 1) if x.dim() == 4 else (1, -1)
        g = (g * _act_mask(y, ctx.relu, ctx.act_max).to(g.dtype)).float()
        dims = (0, 2, 3) if x.dim() == 4 else (0,)
        xhat = (x.float() - mean.view(shape)) * invstd.view(shape)
        g_gamma = (g * xhat).sum(dims)
        g_beta = g.sum(dims)
        if ws > 1:
            pair = torch.stack([g_beta, g_gamma])
            dist.all_reduce(pair)
            g_beta_r, g_gamma_r = pair[0], pair[1]
        else:
            g_beta_r, g_gamma_r = g_beta, g_gamma
        wf = weight.float()
        if ctx.training:
            n = x.numel() / x.shape[1] * ws
            gx = (wf.view(shape) * invstd.view(shape)) * (
                g - g_beta_r.view(shape) / n - xhat * g_gamma_r.view(shape) / n)
        else:
            gx = g * (wf.view(shape) * invstd.view(shape))
        return (gx.to(x.dtype), g_gamma.to(weight.dtype),
                g_beta.to(weight.dtype)) + (None,) * 8


def bn_act(x, weight, bias, running_mean, running_var, training, momentum,
           eps, relu=True, act_max=0.0, sync=False):
    return BnAct.apply(x, weight, bias, running_mean, running_var, training,
                       momentum, eps, relu, act_max, sync)


# ---------------------------------------------------------------------------
# Fused BatchNorm + ReLU + clip + fake-quant (+ channel padding, + max)
# ---------------------------------------------------------------------------


def conv_input_pad_width(x, w, padding=0):
    """Channel count of the padded input copy the noisy conv of ``x`` with
    ``w`` (stride 1) runs on: round8(C) where conv_fwd_fused's patch route
    pads a 16-bit input with C % 8 != 0 itself, else C (no padded copy)."""
    C = x.shape[1]
    if (C % 8 == 0 or not use_native(x, w) or x.element_size() != 2
            or _os.environ.get("NOISYNET_CONV_PAD_SHARE") == "0"):
        return C
    route = ext().conv_fused_route(C, x.shape[2], x.shape[3], w.shape[0],
                                   w.shape[2], w.shape[3], 1, padding,
                                   x.element_size())
    return (C + 7) // 8 * 8 if route == "patch" else C


def bn_act_quant_native(x, running_mean, min_value):
    """Whether bn_act_quant runs its single-kernel forward on ``x``: a 16-bit
    GPU tensor with numel % 4 == 0 (the composition quantises other sizes
    with its scalar kernel, whose roundings the fused kernel does not
    reproduce) and an unsigned range."""
    return (use_native(x) and x.dtype in (torch.bfloat16, torch.float16)
            and x.dim() in (2, 4) and x.numel() > 0 and x.numel() % 4 == 0
            and (running_mean is None or running_mean.dtype == torch.float32)
            and float(min_value) == 0.0)


class BnActQuant(torch.autograd.Function):
    """Training-mode BN + ReLU + clip + fake-quant with ONE forward kernel
    (csrc/bn_act_quant.hip), bit-identical to bn_act -> fake_quant -> max().

    Forward: bn_stats_finalize, then one pass that reads x and writes the
    activation (kept for backward), the quantised tensor with its channels
    zero-padded to ``c_pad``, and its maximum. No unpadded quantised tensor
    is stored: the first output is a [N, C, H, W] view of the padded buffer
    (x's own layout when c_pad == C). Backward is the composition's own pair
    of kernels, ste_mask then bn_act_bwd, on the saved activation."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps, act_max, num_bits, min_value, max_value, stochastic,
                c_pad):
        xc = _nhwc(x) if x.dim() == 4 else x.contiguous()
        empty = torch.empty(0, device=x.device, dtype=torch.float32)
        mean, invstd = ext().bn_stats_finalize(
            xc,
            running_mean if running_mean is not None else empty,
            running_var if running_var is not None else empty,
            float(momentum), float(eps))
        # the seed is drawn where fake_quant draws its own, so every later
        # layer sees the same seed sequence as on the composition
        act, xq_pad, xmax = ext().bn_act_quant_fwd(
            xc, mean, invstd, weight.float().contiguous(),
            bias.float().contiguous(), True, float(act_max), int(num_bits),
            float(min_value), float(max_value), float(stochastic),
            _next_seed(x.device), int(c_pad))
        C = x.shape[1]
        if x.dim() == 4:
            N, _, H, W = x.shape
            xq = xq_pad.view(N, H, W, c_pad)[..., :C].permute(0, 3, 1, 2)
        else:
            xq = xq_pad[:, :C]
        xmax = xmax.to(x.dtype).reshape(())
        ctx.save_for_backward(xc, weight, mean, invstd, act)
        ctx.act_max = float(act_max)
        ctx.q_range = (float(min_value), float(max_value))
        ctx.mark_non_differentiable(xq_pad, xmax)
        return xq, xq_pad, xmax

    @staticmethod
    def backward(ctx, g, _g_pad, _g_max):
        x, weight, mean, invstd, act = ctx.saved_tensors
        gq = ext().ste_mask(g, act, ctx.q_range[0], ctx.q_range[1])
        gx, g_gamma, g_beta = ext().bn_act_bwd(
            gq, x, act, mean, invstd, weight.float().contiguous(), True, True,
            ctx.act_max)
        return (gx, g_gamma.to(weight.dtype),
                g_beta.to(weight.dtype)) + (None,) * 10


def bn_act_quant(x, weight, bias, running_mean, running_var, momentum, eps,
                 act_max, num_bits, min_value, max_value, stochastic=0.0,
                 c_pad=None):
    """Training-mode ``fake_quant(bn_act(x, relu=True, act_max))`` and its
    maximum. Returns ``(xq, x_pad, xq_max)``.

    Tensors that pass bn_act_quant_native take BnActQuant: ``x_pad`` is
    the [rows, c_pad] channel-padded quantised tensor (None when ``c_pad`` is
    None or C) and ``xq`` a view of it; hand both to fused_noisy_conv2d.
    ``c_pad`` comes from conv_input_pad_width. Everything else (CPU, fp32, a
    signed range, numel % 4 != 0) is the composition of the two ops, with
    ``x_pad`` None."""
    C = x.shape[1]
    if bn_act_quant_native(x, running_mean, min_value):
        c_pad = C if c_pad is None else int(c_pad)
        xq, xq_pad, xmax = BnActQuant.apply(
            x, weight, bias, running_mean, running_var, momentum, eps,
            act_max, num_bits, min_value, max_value, stochastic, c_pad)
        return xq, (xq_pad if c_pad != C else None), xmax
    y = bn_act(x, weight, bias, running_mean, running_var, True, momentum,
               eps, relu=True, act_max=act_max)
    xq = fake_quant(y, num_bits, min_value, max_value, stochastic)
    return xq, None, xq.detach().max()


# ---------------------------------------------------------------------------
# Pooling
# ---------------------------------------------------------------------------


class MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if use_native(x):
            y, idx = ext().maxpool2x2_fwd(_nhwc(x))
        else:
            y, idx = F.max_pool2d(x, 2, 2, return_indices=True)
        ctx.save_for_backward(idx)
        ctx.x_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        if use_native(g):
            gx = ext().maxpool2x2_bwd(_nhwc(g), idx, ctx.x_shape[2], ctx.x_shape[3])
        else:
            gx = F.max_unpool2d(g, idx, 2, 2, output_size=ctx.x_shape[2:])
        return gx


def maxpool2x2(x):
    return MaxPool2x2.apply(x)


class MaxPoolNHWC(torch.autograd.Function):
    """Generic k x k / stride / pad max pool (ResNet 3x3 s2 stem etc.)."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        if use_native(x):
            y, code = ext().maxpool_fwd(_nhwc(x), k, stride, pad)
        else:
            y, code = F.max_pool2d(x, k, stride, pad, return_indices=True)
        ctx.save_for_backward(code)
        ctx.meta = (x.shape, k, stride, pad)
        return y

    @staticmethod
    def backward(ctx, g):
        (code,) = ctx.saved_tensors
        x_shape, k, stride, pad = ctx.meta
        if use_native(g):
            gx = ext().maxpool_bwd(_nhwc(g), code, x_shape[2], x_shape[3],
                                   k, stride, pad)
        else:
            # windows overlap when stride < k: accumulate (max_unpool2d
            # overwrites, keeping one window's gradient per cell)
            n, c = x_shape[:2]
            gx = torch.zeros(n, c, x_shape[2] * x_shape[3],
                             dtype=torch.float32, device=g.device)
            gx.scatter_add_(2, code.reshape(n, c, -1),
                            g.reshape(n, c, -1).float())
            gx = gx.view(x_shape).to(g.dtype)
        return gx, None, None, None


def maxpool_nhwc(x, k, stride, pad=0):
    return MaxPoolNHWC.apply(x, k, stride, pad)


class AvgPoolNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        ctx.meta = (x.shape, k, stride, pad)
        if use_native(x):
            return ext().avgpool_fwd(_nhwc(x), k, stride, pad)
        return F.avg_pool2d(x, k, stride, pad)

    @staticmethod
    def backward(ctx, g):
        x_shape, k, stride, pad = ctx.meta
        if use_native(g):
            gx = ext().avgpool_bwd(_nhwc(g), x_shape[2], x_shape[3], k,
                                   stride, pad)
        else:
            # the pool is linear: its f32 autograd gradient at any point.
            # (A conv_transpose of ones with the pool's padding crops the
            # far edge as well and lost the last row/column a window
            # reaches, e.g. 8x8 k3 s2 p1; in a 16-bit dtype its rounded
            # 1/(k*k) also biased every cell.)
            with torch.enable_grad():
                xz = torch.zeros(x_shape, dtype=torch.float32,
                                 device=g.device, requires_grad=True)
                (gx,) = torch.autograd.grad(
                    F.avg_pool2d(xz, k, stride, pad), xz, g.float())
            gx = gx.to(g.dtype)
        return gx, None, None, None


def avgpool_nhwc(x, k, stride, pad=0):
    return AvgPoolNHWC.apply(x, k, stride, pad)


# ---------------------------------------------------------------------------
# Depthwise conv (groups == channels): MobileNetV2 / EfficientNet dw layers
# ---------------------------------------------------------------------------


class DwConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad):
        ctx.stride, ctx.pad = stride, pad
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        if use_native(x, w):
            return ext().dwconv_fwd(
                _nhwc(x), w.contiguous(),
                bias if bias is not None else torch.empty(0, device=x.device,
                                                          dtype=x.dtype),
                stride, pad)
        return F.conv2d(x, w, bias, stride, pad, 1, x.shape[1])

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if use_native(g):
            if ctx.needs_input_grad[0]:
                gx = ext().dwconv_dgrad(_nhwc(g), w.contiguous(), ctx.stride,
                                        ctx.pad, x.shape[2], x.shape[3])
            if ctx.needs_input_grad[1]:
                gw = ext().dwconv_wgrad(_nhwc(g), _nhwc(x), ctx.stride,
                                        ctx.pad, w.shape[2], w.shape[3])
        else:
            if ctx.needs_input_grad[0]:
                gx = torch.nn.grad.conv2d_input(x.shape, w, g, ctx.stride,
                                                ctx.pad, 1, x.shape[1])
            if ctx.needs_input_grad[1]:
                gw = torch.nn.grad.conv2d_weight(x, w.shape, g, ctx.stride,
                                                 ctx.pad, 1, x.shape[1])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None


def depthwise_conv2d(x, w, bias=None, stride=1, padding=0):
    if isinstance(stride, (tuple, list)):
        stride = stride[0]
    if isinstance(padding, (tuple, list)):
        padding = padding[0]
    return DwConv2d.apply(x, w, bias, stride, padding)


# ---------------------------------------------------------------------------
# EfficientNet-family activations (memory-efficient analytic backward)
# ---------------------------------------------------------------------------

_ACT_IDS = {"swish": 0, "mish": 1, "hardswish": 2, "hardsigmoid": 3,
            "sigmoid": 4}


def _act_ref_fwd(x, act):
    if act == "swish":
        return x * torch.sigmoid(x)
    if act == "mish":
        return x * F.softplus(x).tanh()
    if act == "hardswish":
        return x * F.relu6(x + 3.0) / 6.0
    if act == "hardsigmoid":
        return F.relu6(x + 3.0) / 6.0
    return torch.sigmoid(x)


def _act_ref_bwd(g, x, act):
    if act == "swish":
        s = torch.sigmoid(x)
        return g * (s * (1 + x * (1 - s)))
    if act == "mish":
        sp = F.softplus(x)
        tsp = sp.tanh()
        s = torch.sigmoid(x)
        return g * (tsp + x * s * (1 - tsp * tsp))
    if act == "hardswish":
        d = torch.where(x <= -3.0, torch.zeros_like(x),
                        torch.where(x >= 3.0, torch.ones_like(x),
                                    (2 * x + 3.0) / 6.0))
        return g * d
    if act == "hardsigmoid":
        d = ((x > -3.0) & (x < 3.0)).to(g.dtype) / 6.0
        return g * d
    s = torch.sigmoid(x)
    return g * s * (1 - s)


class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        ctx.act = act
        ctx.save_for_backward(x)
        if use_native(x):
            return ext().act_fwd(x, _ACT_IDS[act])
        # f32 arithmetic and one rounding, as the kernel
        return _act_ref_fwd(x.float(), act).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if use_native(x):
            # the C++ wrapper aligns g to x's memory format; a plain
            # .contiguous() here forced an NCHW round-trip of every
            # channels_last activation grad (5.3 ms/step on EffNet-B0)
            return ext().act_bwd(g, x, _ACT_IDS[ctx.act]), None
        return _act_ref_bwd(g.float(), x.float(), ctx.act).to(g.dtype), None


def swish(x):
    return ActFn.apply(x, "swish")


def mish(x):
    return ActFn.apply(x, "mish")


def hard_swish(x):
    return ActFn.apply(x, "hardswish")


def hard_sigmoid(x):
    return ActFn.apply(x, "hardsigmoid")


def sigmoid(x):
    return ActFn.apply(x, "sigmoid")


# ---------------------------------------------------------------------------
# ReLU + clip (standalone, used where BN is off / merged)
# ---------------------------------------------------------------------------


class ReluClip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act_max, relu):
        if use_native(x):
            y = ext().relu_clip_fwd(x, bool(relu), float(act_max))
        else:
            y = F.relu(x) if relu else x
            if act_max > 0:
                y = y.clamp(max=act_max)
        ctx.save_for_backward(y)
        ctx.relu, ctx.act_max = relu, act_max
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        if use_native(y):
            # wrapper aligns g to y's memory format (no NCHW round-trip)
            return (ext().relu_clip_bwd(g, y, bool(ctx.relu),
                                        float(ctx.act_max)), None, None)
        return g * _act_mask(y, ctx.relu, ctx.act_max).to(g.dtype), None, None


def relu_clip(x, act_max=0.0, relu=True):
    return ReluClip.apply(x, act_max, relu)


# ---------------------------------------------------------------------------
# Dropout (Philox in-kernel on GPU)
# ---------------------------------------------------------------------------


class Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        if use_native(x):
            y, mask = ext().dropout_fwd(x, float(p), _next_seed(x.device))
        else:
            mask = (torch.rand_like(x) >= p).to(x.dtype) / (1.0 - p)
            y = x * mask
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def dropout(x, p, training):
    if not training or p <= 0:
        return x
    return Dropout.apply(x, p)


# ---------------------------------------------------------------------------
# Softmax cross-entropy (fused on GPU)
# ---------------------------------------------------------------------------


class SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        if use_native(logits):
            loss, softmax = ext().softmax_xent_fwd(logits.contiguous(), target.contiguous())
        else:
            logp = F.log_softmax(logits.float(), dim=1)
            loss = F.nll_loss(logp, target)
            softmax = logp.exp().to(logits.dtype)
        ctx.save_for_backward(softmax, target)
        return loss

    @staticmethod
    def backward(ctx, g):
        softmax, target = ctx.saved_tensors
        n, c = softmax.shape
        if use_native(softmax):
            if isinstance(g, torch.Tensor) and g.is_cuda:
                # device-resident scale: no host sync (graph-capturable)
                gx = ext().softmax_xent_bwd_t(
                    softmax, target, g.detach().to(torch.float32).reshape(1))
            else:
                gx = ext().softmax_xent_bwd(softmax, target, float(g))
        else:
            onehot = F.one_hot(target, c).to(softmax.dtype)
            gx = (softmax - onehot) * (g / n)
        return gx, None


def cross_entropy(logits, target):
    return SoftmaxXent.apply(logits, target)


# ---------------------------------------------------------------------------
# Fused optimizer steps (no_grad; clamp folded in)
# ---------------------------------------------------------------------------


def _grad_like(param, grad):
    """Raw-layout-match the gradient to the parameter (channels_last conv
    weights on GPU vs standard-contiguous grads, or vice versa)."""
    if param.dim() == 4 and param.is_contiguous(memory_format=torch.channels_last) \
            and not param.is_contiguous():
        return grad.contiguous(memory_format=torch.channels_last)
    return grad.contiguous()


@torch.no_grad()
def sgd_step(param, grad, momentum_buf, lr, momentum, weight_decay, nesterov,
             clamp_min=0.0, clamp_max=0.0):
    """SGD with L2, momentum, nesterov, and post-step weight clamping fused.

    Mirrors torch.optim.SGD semantics + the post-step p.clamp_(-w_max,w_max)
    of noisynet.py:1527-1542.
    """
    if use_native(param):
        ext().sgd_step(param, _grad_like(param, grad), momentum_buf,
                       float(lr), float(momentum),
                       float(weight_decay), bool(nesterov), float(clamp_min),
                       float(clamp_max))
        return
    g = grad
    if weight_decay != 0:
        g = g + weight_decay * param
    if momentum != 0:
        momentum_buf.mul_(momentum).add_(g)
        g = g + momentum * momentum_buf if nesterov else momentum_buf
    param.add_(g, alpha=-lr)
    if clamp_max > clamp_min:
        param.clamp_(clamp_min, clamp_max)


@torch.no_grad()
def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
               weight_decay, clamp_min=0.0, clamp_max=0.0):
    """AdamW (decoupled weight decay) + fused post-step clamp."""
    if use_native(param):
        ext().adamw_step(param, _grad_like(param, grad), exp_avg, exp_avg_sq,
                         int(step), float(lr), float(beta1), float(beta2),
                         float(eps), float(weight_decay), float(clamp_min),
                         float(clamp_max))
        return
    param.mul_(1 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt().add_(eps)
    param.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if clamp_max > clamp_min:
        param.clamp_(clamp_min, clamp_max)


# ---------------------------------------------------------------------------
# Percentile calibration
# ---------------------------------------------------------------------------


def kth_percentile(x, pctl):
    if use_native(x):
        return ext().kth_percentile(x.contiguous().view(-1), float(pctl))
    return ref.kth_percentile(x, pctl)


# ---------------------------------------------------------------------------
# Per-sample (conditionally-parameterized) grouped conv
# ---------------------------------------------------------------------------


def per_sample_conv2d(x, weight, bias=None, stride=1, padding=0, groups=1):
    """Convolution where every sample has its OWN filter bank (CondConv,
    reference conv2d_layers.py:152-240).

    The reference runs this as one grouped conv with batch*groups groups --
    a shape cuDNN special-cases but that maps terribly to grouped-conv
    kernels. Here it is unfold + ONE batched GEMM: im2col columns
    [B, g, L, C/g*R*S] contracted against the per-sample filters
    [B, g, C/g*R*S, K/g] via a single rocBLAS strided-batched GEMM (plain
    library GEMMs are the one sanctioned library path). Fully
    differentiable (double-backward included) through torch autograd.

    x: [B, C, H, W]; weight: [B*K, C/g, R, S] (per-sample filters, sample-
    major as CondConv produces them); returns [B, K, OH, OW].
    """
    B, C, H, W = x.shape
    BK, Cg, R, S = weight.shape
    K = BK // B
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    pd = (padding, padding) if isinstance(padding, int) else tuple(padding)
    OH = (H + 2 * pd[0] - R) // st[0] + 1
    OW = (W + 2 * pd[1] - S) // st[1] + 1
    cols = F.unfold(x, (R, S), padding=pd, stride=st)  # [B, C*R*S, L]
    L = cols.shape[-1]
    g = groups
    # columns laid out [g, C/g*R*S] along dim 1
    cols = cols.view(B, g, Cg * R * S, L)
    w = weight.view(B, g, K // g, Cg * R * S)
    out = torch.matmul(w, cols)                        # [B, g, K/g, L]
    out = out.reshape(B, K, OH, OW)
    if bias is not None:
        out = out + bias.view(B, K, 1, 1)
    return out


# ---------------------------------------------------------------------------
# Squeeze-Excite gating (fused broadcast-scale + per-(b,c) reduce backward)
# ---------------------------------------------------------------------------


_SE_GATES = {'sigmoid': 4, 'hard_sigmoid': 3}


class SeScale(torch.autograd.Function):
    """y = x * gate(s) with per-(batch, channel) logits s [B,C,1,1].

    Replaces the eager broadcast multiply + backward reduce of the SE
    block (reference efficientnet SqueezeExcite, models/efficientnet.py:
    449-466) with one fused pass each way."""

    @staticmethod
    def forward(ctx, x, s, gate_code):
        ctx.gate_code = gate_code
        ctx.save_for_backward(x, s)
        return ext().se_scale_fwd(x, s, gate_code)

    @staticmethod
    def backward(ctx, g):
        x, s = ctx.saved_tensors
        gx, gs = ext().se_scale_bwd(g, x, s, ctx.gate_code)
        return gx, gs.view_as(s), None


def se_scale(x, s, gate='sigmoid'):
    if use_native(x, s) and x.dim() == 4:
        return SeScale.apply(_nhwc(x), s, _SE_GATES[gate])
    gate_fn = torch.sigmoid if gate == 'sigmoid' \
        else lambda t: F.hardsigmoid(t)
    return x * gate_fn(s)


# ---------------------------------------------------------------------------
# Image batch preparation: crop + antialiased resize + mirror + normalise
# ---------------------------------------------------------------------------

_CROP_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _host_int_array(t, dtype, what):
    """Host numpy copy of an index tensor (device tensors are copied back;
    the loaders pass host tensors so their loop never syncs)."""
    import numpy as np
    if isinstance(t, torch.Tensor):
        want = torch.int64 if dtype == np.int64 else torch.int32
        if t.dtype != want:
            raise ValueError('%s must be %s, got %s' % (what, want, t.dtype))
        return t.detach().cpu().numpy()
    a = np.asarray(t)
    if a.dtype != dtype:
        raise ValueError('%s must be %s, got %s' % (what, dtype, a.dtype))
    return a


def check_crop_request(arena_numel, offsets, meta, out_size):
    """Validate host copies of a crop request; raises ValueError.

    An invalid request must never reach the GPU: every bound the kernel
    relies on (box inside the image, window inside the virtual image, image
    inside the arena) is checked here with numpy.
    """
    import numpy as np
    S = int(out_size)
    if S < 1:
        raise ValueError('out_size must be >= 1, got %d' % S)
    if offsets.ndim != 1:
        raise ValueError('offsets must be 1-D')
    if meta.ndim != 2 or meta.shape != (offsets.shape[0], 11):
        raise ValueError('meta must be [B, 11] with B = len(offsets), got %s'
                         % (tuple(meta.shape),))
    if meta.shape[0] == 0:
        return
    m = meta.astype(np.int64)
    H, W, x0, y0, bw, bh, oh, ow, oy, ox, flip = (m[:, i] for i in range(11))

    def need(cond, msg):
        if not bool(np.all(cond)):
            bad = int(np.argmin(cond))
            raise ValueError('crop request sample %d: %s (meta=%s)'
                             % (bad, msg, meta[bad].tolist()))

    need((H >= 1) & (W >= 1), 'image size must be >= 1')
    need((bw >= 1) & (bh >= 1), 'box extent must be >= 1')
    need((x0 >= 0) & (x0 + bw <= W), 'box leaves the image on x')
    need((y0 >= 0) & (y0 + bh <= H), 'box leaves the image on y')
    need((oh >= 1) & (ow >= 1), 'virtual size must be >= 1')
    need((oy >= 0) & (oy + S <= oh), 'window leaves the virtual image on y')
    need((ox >= 0) & (ox + S <= ow), 'window leaves the virtual image on x')
    need((flip == 0) | (flip == 1), 'flip must be 0 or 1')
    need((offsets >= 0) & (offsets + 3 * H * W <= int(arena_numel)),
         'image leaves the arena')


def upload_crop_request(offsets, meta, device, targets=None):
    """One non-blocking upload of (offsets int64[B], meta int32[B, 11]) and,
    for the loaders, the batch's int64 labels.

    All of it lives in one freshly allocated pinned buffer (the caching host
    allocator keeps it alive until the copy has run), viewed on the device
    as the tensors the kernel takes.
    """
    B = int(offsets.shape[0])
    nt = 0 if targets is None else B
    host = torch.empty(2 * (B + nt) + 11 * B, dtype=torch.int32,
                       pin_memory=True)
    host[:2 * B].view(torch.int64).copy_(torch.from_numpy(offsets))
    if nt:
        host[2 * B:4 * B].view(torch.int64).copy_(torch.from_numpy(targets))
    host[2 * (B + nt):].view(B, 11).copy_(torch.from_numpy(meta))
    dev = host.to(device, non_blocking=True)
    off_d = dev[:2 * B].view(torch.int64)
    meta_d = dev[2 * (B + nt):].view(B, 11)
    if nt:
        return off_d, meta_d, dev[2 * B:4 * B].view(torch.int64)
    return off_d, meta_d


def crop_resize_mirror_normalize(arena, offsets, meta, out_size,
                                 mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                                 out_dtype=torch.float32, host_copies=None):
    """Crop, antialiased-bilinear resize, window, mirror, normalise and cast
    a whole batch out of a packed uint8 arena -> [B, 3, S, S] channels_last.

    ``offsets`` (int64[B]) and ``meta`` (int32[B, 11]: H, W, x0, y0, bw, bh,
    oh, ow, oy, ox, flip) are validated on the host before anything is
    launched (ValueError). Pass them as host tensors/arrays in a loop: they
    are then uploaded with one non-blocking copy; device tensors are
    accepted too but cost a copy back for the validation, unless
    ``host_copies=(offsets, meta)`` hands over the numpy arrays they were
    uploaded from.
    """
    import numpy as np
    if not isinstance(arena, torch.Tensor) or arena.dtype != torch.uint8 \
            or arena.dim() != 1:
        raise ValueError('arena must be a 1-D uint8 tensor')
    if out_dtype not in _CROP_DTYPES:
        raise ValueError('out_dtype must be float32, bfloat16 or float16')
    mean = tuple(float(v) for v in mean)
    std = tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
        raise ValueError('mean/std need 3 values each, std > 0')
    for name, t in (('offsets', offsets), ('meta', meta)):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.device != arena.device:
            raise ValueError('%s is on %s but the arena is on %s'
                             % (name, t.device, arena.device))
    if host_copies is not None:
        off_np = _host_int_array(host_copies[0], np.int64, 'offsets')
        meta_np = _host_int_array(host_copies[1], np.int32, 'meta')
        if off_np.shape[0] != offsets.shape[0] \
                or tuple(meta.shape) != tuple(meta_np.shape):
            raise ValueError('host_copies do not match offsets/meta')
    else:
        off_np = _host_int_array(offsets, np.int64, 'offsets')
        meta_np = _host_int_array(meta, np.int32, 'meta')
    check_crop_request(arena.numel(), off_np, meta_np, out_size)

    if use_native(arena):
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda \
                and isinstance(meta, torch.Tensor) and meta.is_cuda:
            off_d, meta_d = offsets.contiguous(), meta.contiguous()
        else:
            off_d, meta_d = upload_crop_request(
                np.ascontiguousarray(off_np), np.ascontiguousarray(meta_np),
                arena.device)
        return ext().crop_resize_mirror_normalize(
            arena.contiguous(), off_d, meta_d, int(out_size), list(mean),
            list(std), _CROP_DTYPES[out_dtype])
    arena_h = arena.cpu() if arena.is_cuda else arena
    out = ref.crop_resize_mirror_normalize(
        arena_h, torch.from_numpy(off_np), torch.from_numpy(meta_np),
        int(out_size), mean, std, out_dtype)
    # NOISYNET_FORCE_REFERENCE with a GPU arena: hand the result back there
    return out.to(arena.device) if arena.is_cuda else out
