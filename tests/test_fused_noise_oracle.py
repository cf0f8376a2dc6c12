"""The fused-noise oracle, checked on the CPU.

The reference path of ops.fused_noisy_conv2d / ops.fused_noisy_linear must
pass the oracle, and seven deliberately wrong fields must each fail it on the
statistic that the defect distorts. That is what shows that the GPU tests
built on the same oracle (test_fused_noise_gpu.py) can fail at all.
"""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

# N, C, H, W, K, R, stride, pad: 542 080 outputs, K = 64 + a ragged 6
SHAPE = (16, 13, 22, 22, 70, 3, 1, 1)
DTYPE = torch.bfloat16
FACTOR = 0.5
MODE = "abs"


@pytest.fixture(scope="module")
def case():
    N, C, H, W, K, R, stride, pad = SHAPE
    inp = fo.make_inputs((N, C, H, W), (K, C, R, R), DTYPE, seed=11)
    refs = fo.conv_refs(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad, MODE)
    gen = torch.Generator().manual_seed(12)
    g = torch.randn(refs.clean.shape, generator=gen, dtype=torch.float64)
    return inp, refs, g


def field(refs, g, sig=None, clean=None):
    """clean + g*sqrt(factor*sig), rounded to the output dtype."""
    sig = refs.sig if sig is None else sig
    clean = refs.clean if clean is None else clean
    return (clean + g * (FACTOR * sig).sqrt()).to(DTYPE)


def report(refs, out):
    return fo.noise_field_report(out, refs.clean, refs.sig, FACTOR)[0]


def test_correct_field_passes(case):
    inp, refs, g = case
    rep = fo.check_noise_field(field(refs, g), refs.clean, refs.sig, FACTOR)
    assert max(rep.values()) <= fo.N_SE


@pytest.mark.parametrize("mode", ["abs", "abs2"])
def test_cpu_reference_conv_passes(mode):
    N, C, H, W, K, R, stride, pad = (4, 13, 22, 22, 70, 3, 1, 1)
    inp = fo.make_inputs((N, C, H, W), (K, C, R, R), DTYPE, seed=21)
    refs = fo.conv_refs(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad, mode)
    torch.manual_seed(22)
    # the CPU branch in fp32 on bf16-representable operands, output rounded
    out = ops.fused_noisy_conv2d(inp.x.float(), inp.wq.float(),
                                 inp.w_raw.float(), inp.bias.float(), stride,
                                 pad, mode, FACTOR).to(DTYPE)
    fo.check_noise_field(out, refs.clean, refs.sig, FACTOR)


@pytest.mark.parametrize("mode", ["abs", "abs2"])
def test_cpu_reference_linear_passes(mode):
    M, Kc, K = 2000, 96, 65
    inp = fo.make_inputs((M, Kc), (K, Kc), DTYPE, seed=31)
    refs = fo.linear_refs(inp.x, inp.wq, inp.w_raw, inp.bias, mode)
    torch.manual_seed(32)
    out = ops.fused_noisy_linear(inp.x.float(), inp.wq.float(),
                                 inp.w_raw.float(), inp.bias.float(), mode,
                                 FACTOR).to(DTYPE)
    fo.check_noise_field(out, refs.clean, refs.sig, FACTOR)


def test_cpu_reference_clean_part_meets_bound():
    # factor 0: the fp32 CPU conv is an fp32-accumulated result too
    N, C, H, W, K, R, stride, pad = (2, 13, 11, 11, 70, 3, 1, 1)
    inp = fo.make_inputs((N, C, H, W), (K, C, R, R), DTYPE, seed=41)
    refs = fo.conv_refs(inp.x, inp.wq, inp.w_raw, inp.bias, stride, pad, MODE)
    out = ops.fused_noisy_conv2d(inp.x.float(), inp.wq.float(),
                                 inp.w_raw.float(), inp.bias.float(), stride,
                                 pad, MODE, 0.0).to(DTYPE)
    fo.assert_within(out, refs.clean,
                     fo.det_bound(refs.clean, refs.A, refs.n, DTYPE), "clean")
    # and a relative defect of 2^-6 is beyond it
    wrong = (out.float() * (1 + 2.0 ** -6)).to(DTYPE)
    assert fo.bound_ratio(wrong, refs.clean, fo.det_bound(
        refs.clean, refs.A, refs.n, DTYPE)) > 1.0


# ---- sabotaged fields: each must fail, on the statistic named -------------


def test_sigma_from_wq_fails_std(case):
    inp, refs, g = case
    N, C, H, W, K, R, stride, pad = SHAPE
    wrong = fo.conv_refs(inp.x, inp.wq, inp.wq, inp.bias, stride, pad, MODE)
    rep = report(refs, field(refs, g, sig=wrong.sig))
    assert rep["std"] > 100


def test_uniform_noise_fails_kurtosis(case):
    inp, refs, g = case
    gen = torch.Generator().manual_seed(13)
    u = (torch.rand(g.shape, generator=gen, dtype=torch.float64) - 0.5) \
        * math.sqrt(12.0)
    rep = report(refs, field(refs, u))
    assert rep["kurtosis"] > 100
    # mean and variance alone cannot tell it from a Gaussian
    assert rep["mean"] <= fo.N_SE and rep["std"] <= fo.N_SE


def test_quad_duplicated_gaussian_fails_lag(case):
    inp, refs, g = case
    dup = g[0::4].repeat_interleave(4, dim=0)[:g.shape[0]]
    rep = report(refs, field(refs, dup))
    assert rep["lag1_m"] > 100
    assert rep["mean"] <= fo.N_SE and rep["kurtosis"] <= fo.N_SE


def test_one_register_10pct_sigma_fails_mod4(case):
    inp, refs, g = case
    g2 = g.clone()
    g2[2::4] *= 1.1           # accumulator register 2 of every quad
    rep = report(refs, field(refs, g2))
    assert rep["std"] > fo.N_SE
    assert rep["mod4_std"] > 2 * fo.N_SE


def test_ragged_tile_variance_fails_channel(case):
    inp, refs, g = case
    g2 = g.clone()
    g2[:, 64:] *= 1.1         # variance x1.21 on the ragged n-tile k >= 64
    rep = report(refs, field(refs, g2))
    assert rep["std"] > fo.N_SE
    assert rep["channel_std"] > 2 * fo.N_SE


def test_dropped_bias_fails_channel_mean(case):
    inp, refs, g = case
    rep = report(refs, field(refs, g, clean=refs.clean - inp.bias.double()))
    assert rep["channel_mean"] > 10 * fo.N_SE


def test_shifted_bias_fails_channel_mean(case):
    inp, refs, g = case
    b = inp.bias.double()
    rep = report(refs, field(refs, g, clean=refs.clean - b + b.roll(1)))
    assert rep["channel_mean"] > 10 * fo.N_SE


def test_check_raises_and_names_the_statistic(case):
    inp, refs, g = case
    g2 = g.clone()
    g2[:, 64:] *= 1.1
    with pytest.raises(AssertionError, match="channel_std"):
        fo.check_noise_field(field(refs, g2), refs.clean, refs.sig, FACTOR)
