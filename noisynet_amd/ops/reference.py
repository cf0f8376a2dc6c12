"""Pure-PyTorch reference implementations of every native op.

These are the numerics oracles for the HIP kernels (tests compare the gfx950
kernels against these in fp32) and the execution path on CPU-only machines.

Semantics follow the reference framework exactly; each function cites the
behaviour it reproduces (file:line into /root/reference/).
"""

import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------
# Fake quantization (UniformQuantize chain)
# ---------------------------------------------------------------------------


def fake_quant_forward(x, num_bits, min_value, max_value, stochastic, gen=None):
    """Clamp-quantize-dequantize with optional stochastic rounding.

    Reproduces the exact in-place chain of hardware_model.py:148-170:
      scale = max((max-min)/(2^b-1), 1e-6)
      q = (x - min)/scale  [+ qmin=0]
      q += U(-stochastic, stochastic)   (if stochastic > 0)
      q = round(clamp(q, 0, 2^b-1))
      out = q*scale + min
    Note: the input is NOT pre-clamped; clamping happens in the quantized
    domain, which is equivalent for the deterministic path.
    """
    qmax = 2.0 ** num_bits - 1.0
    scale = max((max_value - min_value) / qmax, 1e-6)
    q = (x - min_value) / scale
    if stochastic > 0:
        noise = torch.empty_like(q)
        if gen is not None:
            noise.uniform_(-stochastic, stochastic, generator=gen)
        else:
            noise.uniform_(-stochastic, stochastic)
        q = q + noise
    q = q.clamp(0.0, qmax).round()
    return q * scale + min_value


def fake_quant_backward(grad_output, x, min_value, max_value):
    """Saturated STE: zero gradient outside [min_value, max_value].

    hardware_model.py:175-183 (strict inequalities).
    """
    mask = (x <= max_value) & (x >= min_value)
    return grad_output * mask.to(grad_output.dtype)


# ---------------------------------------------------------------------------
# Sigma convolutions / GEMMs for the analog noise model
# ---------------------------------------------------------------------------


def sigma_conv2d(x, weight, mode, stride=1, padding=0):
    """Second conv over transformed |W| used for per-pixel noise variance.

    mode='abs'  -> conv2d(x, |W|)          (hardware_model.py:49)
    mode='abs2' -> conv2d(x, |W|^2 + |W|)  (hardware_model.py:62-65)
    """
    aw = weight.abs()
    if mode == "abs2":
        aw = aw * aw + aw
    return F.conv2d(x, aw, None, stride, padding)


def sigma_linear(x, weight, mode):
    aw = weight.abs()
    if mode == "abs2":
        aw = aw * aw + aw
    return F.linear(x, aw, None)


def vmm_noise(sigmas, factor, gen=None):
    """Gaussian sample with per-element std sqrt(factor * sigmas).

    hardware_model.py:59,81: Normal(0, sqrt(0.1*(w_max/I)*sigmas)).sample().
    ``factor`` is the scalar 0.1*w_max/I (merged DAC) or 0.1*input_max/I.
    """
    s = (factor * sigmas).clamp_min(0).sqrt()
    n = torch.randn(sigmas.shape, device=sigmas.device, dtype=sigmas.dtype, generator=gen)
    return n * s


# ---------------------------------------------------------------------------
# Tiled crossbars: per-block noise and ADC (ops.xbar_noisy_conv2d / _linear)
# ---------------------------------------------------------------------------


def xbar_check_args(sigma_mode, xbar_rows, adc_bits, adc_max):
    """Argument rules shared by the Python wrappers of the tiled-crossbar op."""
    if sigma_mode not in (None, "abs", "abs2"):
        raise ValueError("sigma_mode must be None, 'abs' or 'abs2', got %r"
                         % (sigma_mode,))
    if int(xbar_rows) != xbar_rows or xbar_rows <= 0 or xbar_rows % 32:
        raise ValueError("xbar_rows must be a positive multiple of 32, got %r"
                         % (xbar_rows,))
    if int(adc_bits) != adc_bits or not (adc_bits == 0 or 2 <= adc_bits <= 16):
        raise ValueError("adc_bits must be 0 (ADC off) or 2..16, got %r"
                         % (adc_bits,))
    if adc_bits == 0 and sigma_mode is None:
        raise ValueError("xbar op with neither noise (sigma_mode) nor an ADC "
                         "(adc_bits) is the plain conv/linear")
    if adc_bits > 0 and not isinstance(adc_max, torch.Tensor) \
            and not float(adc_max) > 0:
        raise ValueError("adc_max must be > 0 when adc_bits > 0, got %r"
                         % (adc_max,))


def xbar_adc_params(adc_bits, adc_max, device, unipolar=False):
    """fp32 tensor [step, 1/step] with step = adc_max / Qm, both rounded once
    to fp32 (the values the kernel multiplies with); None with the ADC off.
    ``unipolar`` (differential columns): codes 0..Qu, step = adc_max / Qu with
    Qu = 2^adc_bits - 1."""
    if adc_bits == 0:
        return None
    if unipolar:
        qm = float(2 ** int(adc_bits) - 1)
    else:
        qm = float(2 ** (int(adc_bits) - 1) - 1)
    if isinstance(adc_max, torch.Tensor):
        amax = adc_max.detach().to(device=device, dtype=torch.float32).reshape(1)
    else:
        # a fill, not a host-to-device copy: legal under graph capture
        amax = torch.full((1,), float(adc_max), dtype=torch.float32,
                          device=device)
    step = amax / qm
    return torch.cat([step, 1.0 / step])


def xbar_check_serial_args(in_bits, dac_bits, x_step, dtype, sigma_mode,
                           adc_bits, differential=False):
    """Argument rules of the bit-serial input mode (``dac_bits`` > 0); returns
    the slice count J = ceil(in_bits / dac_bits)."""
    if int(dac_bits) != dac_bits or dac_bits < 1:
        raise ValueError("dac_bits must be 0 (all bits at once) or >= 1, "
                         "got %r" % (dac_bits,))
    if differential:
        raise ValueError("differential columns with bit-serial inputs "
                         "(dac_bits > 0) are not built")
    top = 7 if dtype == torch.bfloat16 else 8
    if int(in_bits) != in_bits or not 1 <= in_bits <= top:
        raise ValueError(
            "in_bits must be 1..%d for %s activations (bf16 does not carry "
            "every 8-bit code), got %r" % (top, dtype, in_bits))
    slices = -(-int(in_bits) // int(dac_bits))
    if slices > 4:
        raise ValueError(
            "in_bits %d at dac_bits %d is %d slices, at most 4 are built; the "
            "smallest dac_bits that works is %d"
            % (in_bits, dac_bits, slices, -(-int(in_bits) // 4)))
    if x_step is None:
        raise ValueError("dac_bits > 0 needs x_step, the activation LSB")
    if not isinstance(x_step, torch.Tensor) and not float(x_step) > 0:
        raise ValueError("x_step must be > 0, got %r" % (x_step,))
    if adc_bits == 0 and sigma_mode is None:
        raise ValueError("xbar op with neither noise (sigma_mode) nor an ADC "
                         "(adc_bits): bit-serial inputs have nothing to act on")
    return slices


def xbar_dac_params(x_step, device):
    """fp32 tensor [x_step, 1/x_step], both rounded once to fp32 (the values
    the kernel multiplies with). ``x_step`` is a number or a 1-element tensor
    (then it must be positive; it is not read back to check)."""
    if isinstance(x_step, torch.Tensor):
        xs = x_step.detach().to(device=device, dtype=torch.float32).reshape(1)
    else:
        # a fill, not a host-to-device copy: legal under graph capture
        xs = torch.full((1,), float(x_step), dtype=torch.float32,
                        device=device)
    return torch.cat([xs, 1.0 / xs])


def xbar_check_cell_args(w_bits, cell_bits, w_step, w_min, sigma_mode,
                         adc_bits, differential=False, dac_bits=0):
    """Argument rules of the bit-sliced weight mode (``cell_bits`` > 0);
    returns the slice count T = ceil(w_bits / cell_bits)."""
    if int(cell_bits) != cell_bits or not 1 <= cell_bits <= 4:
        raise ValueError("cell_bits must be 0 (one analog cell per weight) or "
                         "1..4, got %r" % (cell_bits,))
    if differential or dac_bits:
        raise ValueError(
            "bit-sliced weights (cell_bits > 0) cannot be combined with "
            "differential=True or dac_bits > 0: T * J accumulator sets per "
            "output do not fit the kernel's registers, and W+ / W- columns "
            "per weight slice are a follow-up")
    if int(w_bits) != w_bits or not 1 <= w_bits <= 8:
        raise ValueError("w_bits must be 1..8, got %r" % (w_bits,))
    slices = -(-int(w_bits) // int(cell_bits))
    if slices > 4:
        raise ValueError(
            "w_bits %d at cell_bits %d is %d slices, at most 4 are built; the "
            "smallest cell_bits that works is %d"
            % (w_bits, cell_bits, slices, -(-int(w_bits) // 4)))
    if w_step is None or w_min is None:
        raise ValueError("cell_bits > 0 needs w_step and w_min, the weight "
                         "quantiser's grid w = w_min + code * w_step")
    if not isinstance(w_step, torch.Tensor) and not float(w_step) > 0:
        raise ValueError("w_step must be > 0, got %r" % (w_step,))
    if adc_bits == 0 and sigma_mode is None:
        raise ValueError("xbar op with neither noise (sigma_mode) nor an ADC "
                         "(adc_bits): bit-sliced weights have nothing to act "
                         "on")
    return slices


def xbar_cell_params(w_step, w_min, device):
    """fp32 tensor [w_step, 1/w_step, w_min], each rounded once to fp32 (the
    values the kernel computes with). ``w_step`` / ``w_min`` are numbers or
    1-element tensors (w_step must then be positive; it is not read back)."""
    def one(v):
        if isinstance(v, torch.Tensor):
            return v.detach().to(device=device, dtype=torch.float32).reshape(1)
        # a fill, not a host-to-device copy: legal under graph capture
        return torch.full((1,), float(v), dtype=torch.float32, device=device)
    ws, wm = one(w_step), one(w_min)
    return torch.cat([ws, 1.0 / ws, wm])


def xbar_check_program_args(sigma, p_stuck_off, p_stuck_on):
    """Argument rules of the cell model of xbar_program_cells."""
    if not float(sigma) >= 0:
        raise ValueError("sigma (cell conductance variation) must be >= 0, "
                         "got %r" % (sigma,))
    if not float(p_stuck_off) >= 0:
        raise ValueError("p_stuck_off must be >= 0, got %r" % (p_stuck_off,))
    if not float(p_stuck_on) >= 0:
        raise ValueError("p_stuck_on must be >= 0, got %r" % (p_stuck_on,))
    if float(p_stuck_off) + float(p_stuck_on) > 1:
        raise ValueError("p_stuck_off + p_stuck_on must be <= 1, got %r"
                         % (float(p_stuck_off) + float(p_stuck_on),))


def xbar_program_cells(wq, w_bits, cell_bits, cell, sigma=0.0,
                       p_stuck_off=0.0, p_stuck_on=0.0, gen=None):
    """Program a layer's weight codes onto imperfect cells: the CPU twin of
    the HIP kernel xbar_program_cells_kernel. ``wq`` is a conv filter
    [K, C, R, S] or a linear weight [K, n]; the result is G[T, K, n] in the
    dtype of ``wq`` with the rows in crossbar order (r, s, c), c fastest:
        code = clamp(rint((f32(wq) - w_min) * (1/w_step)), 0, 2^B - 1)
        d_t  = (code >> t*E) & (2^E - 1)
        d'_t = 0 with probability p_stuck_off (stuck at the high-resistance
               state), 2^E - 1 with probability p_stuck_on (stuck on: the top
               level of an E-bit cell), d_t otherwise
        G_t  = round_to_dtype(max(d'_t * (1 + sigma * z), 0)),  z ~ N(0, 1)
    in fp32 with the one rounding, one (u, z) pair per cell. The variation is
    multiplicative and Gaussian, clamped at zero: an off cell stays off and a
    stuck-on cell varies like any other. Log-normal variation and additive
    HRS leakage are not modelled. The draws come from ``gen`` (a
    torch.Generator): the kernel's distribution on another stream."""
    xbar_check_program_args(sigma, p_stuck_off, p_stuck_on)
    E, B = int(cell_bits), int(w_bits)
    T = -(-B // E)
    wqm = xbar_weight_rows(wq.detach())
    inv_w_step, w_min = cell[1], cell[2]
    code = torch.round((wqm.float() - w_min) * inv_w_step)
    code = code.clamp(0, float(2 ** B - 1)).to(torch.int32)
    shape = (T,) + tuple(wqm.shape)
    u = torch.rand(shape, dtype=torch.float32, device=wqm.device,
                   generator=gen)
    z = torch.randn(shape, dtype=torch.float32, device=wqm.device,
                    generator=gen)
    d = torch.stack([((code >> (t * E)) & (2 ** E - 1)).float()
                     for t in range(T)])
    top = float(2 ** E - 1)
    p_off, p_on = float(p_stuck_off), float(p_stuck_on)
    d = torch.where(u < p_off, torch.zeros_like(d),
                    torch.where(u < p_off + p_on, torch.full_like(d, top), d))
    return (d * (1.0 + float(sigma) * z)).clamp_min(0).to(wq.dtype)


def xbar_conv_rows(x, R, S, stride, padding):
    """im2col matrix [N*OH*OW, R*S*C] of an NCHW input with the contraction
    index in the filter's memory order (r, s, c), c fastest -- the crossbar
    row order. Padding positions are zeros."""
    N, C = x.shape[0], x.shape[1]
    cols = F.unfold(x, (R, S), padding=padding, stride=stride)  # (c, r, s)
    L = cols.shape[-1]
    cols = cols.view(N, C, R * S, L).permute(0, 3, 2, 1)        # n, l, rs, c
    return cols.reshape(N * L, R * S * C)


def xbar_weight_rows(w):
    """[K, C, R, S] filter -> [K, R*S*C] in the (r, s, c) row order."""
    if w.dim() == 2:
        return w
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def xbar_vmm(xm, wqm, wrm, bias, sigma_mode, factor, xbar_rows, adc_bits,
             adc, gen=None, stats=None, differential=False, dac=None,
             in_bits=0, dac_bits=0, cell=None, w_bits=0, cell_bits=0,
             cells=None):
    """Blocked analog VMM on row matrices: xm [M, n], wqm / wrm [K, n].

    Block b covers rows [b*xbar_rows, min((b+1)*xbar_rows, n)). Per block
        p_b = x_b @ wq_b^T                       s_b = max(x_b @ f(|w_raw,b|)^T, 0)
        v_b = p_b + eps_b * sqrt(factor * s_b)   (eps_b iid N(0,1) per block)
        q_b = step * clamp(rint(v_b * (1/step)), -Qm, Qm)
    and out = sum_b q_b + bias, all in fp32 (b ascending). ``adc`` is the
    [step, 1/step] tensor of xbar_adc_params (None = ADC off, q_b = v_b);
    sigma_mode None = noise off. ``stats`` (a dict) receives the telemetry
    sums: sigma_abs, abs_noise (of the summed block noises), max_y (clean,
    with bias), clipped (count of |rint(v_b/step)| > Qm), n_partials and
    partial_absmax (max |v_b|). Returns fp32 [M, K].

    ``differential`` runs every block on two columns (see _xbar_vmm_diff);
    ``dac_bits`` > 0 streams the input in slices (see _xbar_vmm_serial);
    ``cell_bits`` > 0 spreads the weight code over columns (see
    _xbar_vmm_cells); ``cells`` then hands it the programmed conductances
    G[T, K, n] of xbar_program_cells in place of the ideal digits."""
    if cells is not None and not cell_bits:
        raise ValueError("cells (programmed conductances) needs cell_bits > 0")
    if cell_bits:
        if differential or dac_bits:
            raise ValueError("bit-sliced weights (cell_bits > 0) cannot be "
                             "combined with differential columns or "
                             "bit-serial inputs")
        return _xbar_vmm_cells(xm, wqm, bias, sigma_mode, factor, xbar_rows,
                               adc_bits, adc, cell, w_bits, cell_bits, gen,
                               stats, cells)
    if dac_bits:
        if differential:
            raise ValueError("differential columns with bit-serial inputs "
                             "(dac_bits > 0) are not built")
        return _xbar_vmm_serial(xm, wqm, wrm, bias, sigma_mode, factor,
                                xbar_rows, adc_bits, adc, dac, in_bits,
                                dac_bits, gen, stats)
    if differential:
        return _xbar_vmm_diff(xm, wqm, wrm, bias, sigma_mode, factor,
                              xbar_rows, adc_bits, adc, gen, stats)
    xm, wqm = xm.float(), wqm.float()
    n = xm.shape[1]
    M, K = xm.shape[0], wqm.shape[0]
    out = torch.zeros(M, K, dtype=torch.float32, device=xm.device)
    if sigma_mode is not None:
        aw = wrm.float().abs()
        fw = aw * aw + aw if sigma_mode == "abs2" else aw
        factor = torch.as_tensor(factor, dtype=torch.float32, device=xm.device)
    if adc is not None:
        step, inv_step = adc[0], adc[1]
        qm = float(2 ** (int(adc_bits) - 1) - 1)
    if stats is not None:
        clean = torch.zeros_like(out)
        noise_tot = torch.zeros_like(out)
        sig_abs = out.new_zeros(())
        clipped = 0
        absmax = out.new_zeros(())
        nblk = 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        p = xb @ wqm[:, k0:k1].t()
        v = p
        if sigma_mode is not None:
            s = (xb @ fw[:, k0:k1].t()).clamp_min(0)
            eps = torch.randn(p.shape, dtype=torch.float32, device=p.device,
                              generator=gen)
            nb = eps * (factor * s).sqrt()
            v = p + nb
        if adc is not None:
            t = torch.round(v * inv_step)
            q = step * t.clamp(-qm, qm)
        else:
            q = v
        out = out + q
        if stats is not None:
            nblk += 1
            clean = clean + p
            absmax = torch.maximum(absmax, v.abs().max())
            if sigma_mode is not None:
                noise_tot = noise_tot + nb
                sig_abs = sig_abs + (xb @ aw[:, k0:k1].t()).sum()
            if adc is not None:
                clipped = clipped + (t.abs() > qm).sum()
    if bias is not None:
        out = out + bias.float()
    if stats is not None:
        if bias is not None:
            clean = clean + bias.float()
        stats.update(sigma_abs=sig_abs, abs_noise=noise_tot.abs().sum(),
                     max_y=clean.max(), clipped=clipped,
                     n_partials=nblk * M * K, partial_absmax=absmax)
    return out


def _xbar_vmm_diff(xm, wqm, wrm, bias, sigma_mode, factor, xbar_rows,
                   adc_bits, adc, gen=None, stats=None):
    """xbar_vmm on differential columns: the positive and the negative part of
    the weights sit on two columns with independent noise and unipolar ADCs.
        wq+ = max(wq, 0)   wq- = max(-wq, 0)    f+- = f(|w_raw|) by sign(w_raw)
        p+- = x_b @ wq+-^T                      s+- = max(x_b @ f+-^T, 0)
        v+- = p+- + eps+- * sqrt(factor * s+-)
        q+- = step * clamp(rint(v+- * (1/step)), 0, Qu),  Qu = 2^adc_bits - 1
    and out = sum_b (q+ - q-) + bias. ``stats``: clipped counts column values
    with rint(v/step) > Qu or < 0, n_partials is 2 * nblocks * M * K,
    partial_absmax the max |v+-|, abs_noise uses noise+ - noise-. Meant for
    non-negative x; the sign of x is not inspected."""
    xm, wqm = xm.float(), wqm.float()
    n = xm.shape[1]
    M, K = xm.shape[0], wqm.shape[0]
    out = torch.zeros(M, K, dtype=torch.float32, device=xm.device)
    wqs = (wqm.clamp_min(0), (-wqm).clamp_min(0))
    if sigma_mode is not None:
        wr = wrm.float()
        aw = wr.abs()
        fw = aw * aw + aw if sigma_mode == "abs2" else aw
        zero = torch.zeros_like(fw)
        fws = (torch.where(wr > 0, fw, zero), torch.where(wr < 0, fw, zero))
        factor = torch.as_tensor(factor, dtype=torch.float32, device=xm.device)
    if adc is not None:
        step, inv_step = adc[0], adc[1]
        qu = float(2 ** int(adc_bits) - 1)
    if stats is not None:
        clean = torch.zeros_like(out)
        noise_tot = torch.zeros_like(out)
        sig_abs = out.new_zeros(())
        clipped = 0
        absmax = out.new_zeros(())
        nblk = 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        qs = []
        for col in range(2):          # the positive column draws first
            p = xb @ wqs[col][:, k0:k1].t()
            v = p
            if sigma_mode is not None:
                s = (xb @ fws[col][:, k0:k1].t()).clamp_min(0)
                eps = torch.randn(p.shape, dtype=torch.float32,
                                  device=p.device, generator=gen)
                nb = eps * (factor * s).sqrt()
                v = p + nb
            if adc is not None:
                t = torch.round(v * inv_step)
                q = step * t.clamp(0, qu)
            else:
                q = v
            qs.append(q)
            if stats is not None:
                sgn = 1.0 if col == 0 else -1.0
                clean = clean + sgn * p
                absmax = torch.maximum(absmax, v.abs().max())
                if sigma_mode is not None:
                    noise_tot = noise_tot + sgn * nb
                if adc is not None:
                    clipped = clipped + ((t > qu) | (t < 0)).sum()
        out = out + (qs[0] - qs[1])
        if stats is not None:
            nblk += 1
            if sigma_mode is not None:
                sig_abs = sig_abs + (xb @ aw[:, k0:k1].t()).sum()
    if bias is not None:
        out = out + bias.float()
    if stats is not None:
        if bias is not None:
            clean = clean + bias.float()
        stats.update(sigma_abs=sig_abs, abs_noise=noise_tot.abs().sum(),
                     max_y=clean.max(), clipped=clipped,
                     n_partials=2 * nblk * M * K, partial_absmax=absmax)
    return out


def _xbar_vmm_serial(xm, wqm, wrm, bias, sigma_mode, factor, xbar_rows,
                     adc_bits, adc, dac, in_bits, dac_bits, gen=None,
                     stats=None):
    """xbar_vmm with bit-serial inputs: the activation is an ``in_bits``-bit
    code on the grid x_step (``dac`` = [x_step, 1/x_step] of xbar_dac_params)
    and reaches the rows ``dac_bits`` = D bits per cycle, J = ceil(B/D) slices,
    each with its own current, noise draw and ADC conversion:
        code = clamp(rint(x * (1/x_step)), 0, 2^B - 1)
        d_j  = (code >> j*D) & (2^D - 1)                       j = 0..J-1
        p_bj = x_step * (d_j @ wq_b^T)    s_bj = max(x_step * (d_j @ f_b^T), 0)
        v_bj = p_bj + eps_bj * sqrt(factor * s_bj)
        q_bj = step * clamp(rint(v_bj * (1/step)), -Qm, Qm)
    and out = sum_b sum_j 2^(jD) q_bj + bias in fp32 (b ascending, j ascending
    inside b). Negative and off-grid inputs are re-quantised to the grid.
    ``stats``: sigma_abs = sum 2^(jD) x_step (d_j @ |w_raw|^T), abs_noise uses
    the shift-added noises, max_y the clean shift-added sum with bias, clipped
    counts over all (b, j) partials, n_partials = J * nblocks * M * K and
    partial_absmax = max |v_bj| -- the figure to size a per-slice adc_max
    from."""
    D, B = int(dac_bits), int(in_bits)
    J = -(-B // D)
    x_step, inv_x_step = dac[0], dac[1]
    code = torch.round(xm.float() * inv_x_step).clamp(0, float(2 ** B - 1))
    code = code.to(torch.int32)
    wqm = wqm.float()
    n = xm.shape[1]
    M, K = xm.shape[0], wqm.shape[0]
    out = torch.zeros(M, K, dtype=torch.float32, device=xm.device)
    if sigma_mode is not None:
        aw = wrm.float().abs()
        fw = aw * aw + aw if sigma_mode == "abs2" else aw
        factor = torch.as_tensor(factor, dtype=torch.float32, device=xm.device)
    if adc is not None:
        step, inv_step = adc[0], adc[1]
        qm = float(2 ** (int(adc_bits) - 1) - 1)
    if stats is not None:
        clean = torch.zeros_like(out)
        noise_tot = torch.zeros_like(out)
        sig_abs = out.new_zeros(())
        clipped = 0
        absmax = out.new_zeros(())
        nblk = 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        for j in range(J):
            shift = float(2 ** (j * D))
            dj = ((code[:, k0:k1] >> (j * D)) & (2 ** D - 1)).float()
            p = x_step * (dj @ wqm[:, k0:k1].t())
            v = p
            if sigma_mode is not None:
                s = (x_step * (dj @ fw[:, k0:k1].t())).clamp_min(0)
                eps = torch.randn(p.shape, dtype=torch.float32,
                                  device=p.device, generator=gen)
                nb = eps * (factor * s).sqrt()
                v = p + nb
            if adc is not None:
                t = torch.round(v * inv_step)
                q = step * t.clamp(-qm, qm)
            else:
                q = v
            out = out + shift * q
            if stats is not None:
                clean = clean + shift * p
                absmax = torch.maximum(absmax, v.abs().max())
                if sigma_mode is not None:
                    noise_tot = noise_tot + shift * nb
                    sig_abs = sig_abs + shift * x_step \
                        * (dj @ aw[:, k0:k1].t()).sum()
                if adc is not None:
                    clipped = clipped + (t.abs() > qm).sum()
        if stats is not None:
            nblk += 1
    if bias is not None:
        out = out + bias.float()
    if stats is not None:
        if bias is not None:
            clean = clean + bias.float()
        stats.update(sigma_abs=sig_abs, abs_noise=noise_tot.abs().sum(),
                     max_y=clean.max(), clipped=clipped,
                     n_partials=J * nblk * M * K, partial_absmax=absmax)
    return out


def _xbar_vmm_cells(xm, wqm, bias, sigma_mode, factor, xbar_rows, adc_bits,
                    adc, cell, w_bits, cell_bits, gen=None, stats=None,
                    cells=None):
    """xbar_vmm with bit-sliced weights: a cell holds ``cell_bits`` = E bits,
    so the ``w_bits`` = B bit offset-binary code of a weight on the grid
    w = w_min + code * w_step (``cell`` = [w_step, 1/w_step, w_min] of
    xbar_cell_params) is spread over T = ceil(B/E) columns, each with its own
    current, noise draw and UNIPOLAR ADC conversion:
        code = clamp(rint((wq - w_min) * (1/w_step)), 0, 2^B - 1)
        d_t  = (code >> t*E) & (2^E - 1)                       t = 0..T-1
        p_bt = w_step * (x_b @ d_t^T)
        s_bt = max(p_bt, 0)                                    (abs)
             = max(w_step^2 * (x_b @ (d_t^2)^T) + p_bt, 0)     (abs2)
        v_bt = p_bt + eps_bt * sqrt(factor * s_bt)
        q_bt = step * clamp(rint(v_bt * (1/step)), 0, Qu),  Qu = 2^adc_bits - 1
        X_b  = sum of the block's inputs
    and out = sum_b (sum_t 2^(tE) q_bt + w_min * X_b) + bias in fp32 (b
    ascending, t ascending inside b, then the block's offset). The
    conductances are the digits: w_raw is not used. ``stats``: sigma_abs =
    sum p_bt (the current the cells draw, not shift-weighted), abs_noise uses
    the shift-added noises, max_y the clean shift-added sum with the offset
    and the bias, clipped counts the (b, t) partials with rint(v/step) > Qu or
    < 0, n_partials = T * nblocks * M * K and partial_absmax = max |v_bt| --
    the figure to size the per-slice, unipolar adc_max from.

    ``cells`` = G[T, K, n] (xbar_program_cells; digit units, a 16-bit or fp32
    dtype) replaces the digits: G_t stands for d_t and
    round_to_dtype(f32(G_t)^2) for d_t^2; nothing else changes."""
    E, B = int(cell_bits), int(w_bits)
    T = -(-B // E)
    if cells is not None and tuple(cells.shape) != (T,) + tuple(wqm.shape):
        raise ValueError("cells must have the shape %r (slices, output "
                         "columns, crossbar rows), got %r"
                         % ((T,) + tuple(wqm.shape), tuple(cells.shape)))
    w_step, inv_w_step, w_min = cell[0], cell[1], cell[2]
    w_step2 = w_step * w_step
    code = torch.round((wqm.float() - w_min) * inv_w_step)
    code = code.clamp(0, float(2 ** B - 1)).to(torch.int32)
    xm = xm.float()
    n = xm.shape[1]
    M, K = xm.shape[0], wqm.shape[0]
    out = torch.zeros(M, K, dtype=torch.float32, device=xm.device)
    if sigma_mode is not None:
        factor = torch.as_tensor(factor, dtype=torch.float32, device=xm.device)
    if adc is not None:
        step, inv_step = adc[0], adc[1]
        qu = float(2 ** int(adc_bits) - 1)
    if stats is not None:
        clean = torch.zeros_like(out)
        noise_tot = torch.zeros_like(out)
        sig_abs = out.new_zeros(())
        clipped = 0
        absmax = out.new_zeros(())
        nblk = 0
    for k0 in range(0, n, xbar_rows):
        k1 = min(k0 + xbar_rows, n)
        xb = xm[:, k0:k1]
        for t in range(T):
            shift = float(2 ** (t * E))
            if cells is None:
                dt = ((code[:, k0:k1] >> (t * E)) & (2 ** E - 1)).float()
                dt2 = dt * dt
            else:
                dt = cells[t][:, k0:k1].float()
                dt2 = (dt * dt).to(cells.dtype).float()
            p = w_step * (xb @ dt.t())
            v = p
            if sigma_mode is not None:
                s = p
                if sigma_mode == "abs2":
                    s = w_step2 * (xb @ dt2.t()) + p
                s = s.clamp_min(0)
                eps = torch.randn(p.shape, dtype=torch.float32,
                                  device=p.device, generator=gen)
                nb = eps * (factor * s).sqrt()
                v = p + nb
            if adc is not None:
                c = torch.round(v * inv_step)
                q = step * c.clamp(0, qu)
            else:
                q = v
            out = out + shift * q
            if stats is not None:
                clean = clean + shift * p
                absmax = torch.maximum(absmax, v.abs().max())
                if sigma_mode is not None:
                    noise_tot = noise_tot + shift * nb
                    sig_abs = sig_abs + p.sum()
                if adc is not None:
                    clipped = clipped + ((c > qu) | (c < 0)).sum()
        off = w_min * xb.sum(dim=1, keepdim=True)
        out = out + off
        if stats is not None:
            clean = clean + off
            nblk += 1
    if bias is not None:
        out = out + bias.float()
    if stats is not None:
        if bias is not None:
            clean = clean + bias.float()
        stats.update(sigma_abs=sig_abs, abs_noise=noise_tot.abs().sum(),
                     max_y=clean.max(), clipped=clipped,
                     n_partials=T * nblk * M * K, partial_absmax=absmax)
    return out


# ---------------------------------------------------------------------------
# Fused BN + activation (reference composition)
# ---------------------------------------------------------------------------


def bn_stats(x):
    """Per-channel biased mean/var over (N, H, W) for NCHW or (N,) for NC."""
    if x.dim() == 4:
        dims = (0, 2, 3)
    else:
        dims = (0,)
    mean = x.mean(dim=dims)
    var = x.var(dim=dims, unbiased=False)
    return mean, var


def bn_act_forward(x, weight, bias, mean, invstd, act_max=0.0, relu=True):
    """y = gamma*(x-mean)*invstd+beta, then ReLU, then clamp(<=act_max)."""
    shape = (1, -1, 1, 1) if x.dim() == 4 else (1, -1)
    y = (x - mean.view(shape)) * invstd.view(shape)
    if weight is not None:
        y = y * weight.view(shape)
    if bias is not None:
        y = y + bias.view(shape)
    if relu:
        y = F.relu(y)
    if act_max > 0:
        y = y.clamp(max=act_max)
    return y


# ---------------------------------------------------------------------------
# Elementwise perturbations
# ---------------------------------------------------------------------------


def mult_uniform_noise(x, noise, gen=None):
    """out = x + x*U(-noise, +noise): AddNoise fwd (hardware_model.py:293-301)
    and distort_weights (main.py:372-377)."""
    u = torch.empty_like(x)
    if gen is not None:
        u.uniform_(-noise, noise, generator=gen)
    else:
        u.uniform_(-noise, noise)
    return x + x * u


# ---------------------------------------------------------------------------
# Percentile (kthvalue) calibration
# ---------------------------------------------------------------------------


def kth_percentile(x, pctl):
    """k-th order statistic matching torch.kthvalue semantics used at
    hardware_model.py:233-249: k = int(numel * pctl / 100)."""
    flat = x.flatten()
    k = int(flat.numel() * pctl / 100.0)
    k = max(1, min(k, flat.numel()))
    val, _ = torch.kthvalue(flat.float(), k)
    return val.to(x.dtype)


# ---------------------------------------------------------------------------
# Pooling / loss (reference path = plain torch)
# ---------------------------------------------------------------------------


def maxpool2x2(x):
    return F.max_pool2d(x, 2, 2)


def softmax_xent(logits, target):
    return F.cross_entropy(logits, target)


# ---------------------------------------------------------------------------
# Image batch preparation (crop -> antialiased resize -> window -> mirror ->
# normalise), the oracle for csrc/image_pipeline.hip
# ---------------------------------------------------------------------------


def crop_resize_mirror_normalize(arena, offsets, meta, out_size, mean, std,
                                 out_dtype=torch.float32):
    """Per-sample ``F.interpolate(..., antialias=True)`` composition.

    ``arena`` is 1-D uint8 (images packed HWC RGB), ``offsets`` int64[B],
    ``meta`` int32[B, 11] = H, W, x0, y0, bw, bh, oh, ow, oy, ox, flip.
    The box is resized to (oh, ow), the out_size window at (oy, ox) is taken,
    mirrored on x when flip is set, then ``(v - mean) / std`` on the [0, 1]
    values. Returns [B, 3, S, S] channels_last in ``out_dtype`` (replaces the
    reference's DALI Resize + CropMirrorNormalize, utils.py:63-116).
    """
    S = int(out_size)
    B = int(offsets.shape[0])
    mean_t = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    out = torch.empty((B, 3, S, S), dtype=torch.float32)
    for b in range(B):
        H, W, x0, y0, bw, bh, oh, ow, oy, ox, flip = (int(v) for v in meta[b])
        off = int(offsets[b])
        img = arena[off:off + 3 * H * W].view(H, W, 3)
        box = img[y0:y0 + bh, x0:x0 + bw].permute(2, 0, 1).float() / 255.0
        r = F.interpolate(box[None], size=(oh, ow), mode='bilinear',
                          antialias=True, align_corners=False)[0]
        r = r[:, oy:oy + S, ox:ox + S]
        if flip:
            r = r.flip(-1)
        out[b] = (r - mean_t) / std_t
    return out.to(out_dtype).contiguous(memory_format=torch.channels_last)
