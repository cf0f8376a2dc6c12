"""Fused noisy conv / linear on every dispatch route against the fp64 oracle.

    out = conv(x, wq) + bias + N(0, sqrt(factor * conv(x, f(|w_raw|))))

Every case uses wq != w_raw (scales 0.2 and 0.05) and, unless it says
otherwise, a bias. The shape tables hold the smallest shapes that can still go
wrong (M no multiple of 64, K no multiple of 16 or 64, odd C, a strided and a
padded case); every row asserts the route it is meant to take. The bounds are
derived in fused_noise_oracle.py, not tuned.
"""

import math
import os
import sys
from functools import lru_cache

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_noise_oracle as fo  # noqa: E402
from noisynet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
ALL = (BF16, FP16, FP32)
HALF = (BF16, FP16)
MODES = ("abs", "abs2")
MODE_INT = {"abs": 1, "abs2": 2}
FACTOR = 0.5
NOISE_OUTPUTS = 1 << 17     # at least this many z-scores per noise field

# relative error of tele[0] (sum of sigma_abs) against the fp64 sum. The
# kernels add block partials with float atomics, so no tight bound can be
# derived. Largest value measured on MI355X over every row, dtype, mode and
# entry point of this file: 2.8e-7 (stream 1x16x56x56x24 fp16, sigma-only);
# the bound is 10x that, and may never exceed the 2 % of test_ops_gpu.py.
TELE0_REL = 2.8e-6

# (route, dtypes, (N, C, H, W, K, R, stride, pad))
CONV_ROWS = [
    ("patch", ALL, (3, 13, 11, 11, 70, 3, 1, 1)),
    ("patch", ALL, (2, 24, 15, 15, 20, 3, 2, 1)),
    ("col_smallk", HALF, (3, 3, 15, 15, 65, 5, 1, 0)),
    ("col_smallk", HALF, (2, 8, 9, 9, 20, 2, 1, 0)),
    ("col_gemm", ALL, (2, 8, 10, 10, 16, 3, 1, 0)),
    ("col_gemm", ALL, (2, 3, 15, 15, 100, 5, 1, 0)),
    ("stream", ALL, (2, 40, 7, 7, 70, 1, 1, 0)),
    ("stream", HALF, (1, 16, 56, 56, 24, 3, 1, 1)),
    ("stream", HALF, (1, 16, 56, 56, 24, 3, 2, 1)),
    ("stream", (FP32,), (1, 16, 40, 40, 24, 3, 1, 1)),
]
# (route, dtypes, (M, Kc, K))
LINEAR_ROWS = [
    ("smallk", HALF, (200, 96, 65)),
    ("smallk", HALF, (70, 32, 96)),
    ("gemm", ALL, (70, 390, 10)),
    ("gemm", ALL, (130, 200, 100)),
]


def _name(dtype):
    return str(dtype).replace("torch.", "")


class Case:
    """One table row at one dtype: inputs, fp64 references, kernel calls."""

    def __init__(self, kind, route, shape, dtype):
        self.kind, self.route, self.shape, self.dtype = kind, route, shape, dtype
        self.id = "%s-%s-%s-%s" % (kind, route, "x".join(map(str, shape)),
                                   _name(dtype))

    # -- geometry ----------------------------------------------------------
    def shapes(self, outputs=0):
        """(x shape, w shape) with the batch grown to >= ``outputs`` outputs
        (kept off the multiples of the 64-row tile)."""
        if self.kind == "conv":
            N, C, H, W, K, R, stride, pad = self.shape
            oh = (H + 2 * pad - R) // stride + 1
            ow = (W + 2 * pad - R) // stride + 1
            N = max(N, -(-outputs // (oh * ow * K)))
            return (N, C, H, W), (K, C, R, R)
        M, Kc, K = self.shape
        M = max(M, -(-outputs // K) + 3)
        return (M, Kc), (K, Kc)

    @property
    def n(self):
        """contraction length for the summation bound; a conv also counts one
        partial sum per filter tap (the kernels add tap by tap)."""
        if self.kind == "conv":
            N, C, H, W, K, R, stride, pad = self.shape
            return C * R * R + R * R
        return self.shape[1]

    def actual_route(self):
        es = torch.empty(0, dtype=self.dtype).element_size()
        if self.kind == "conv":
            N, C, H, W, K, R, stride, pad = self.shape
            return ops.ext().conv_fused_route(C, H, W, K, R, R, stride, pad, es)
        M, Kc, K = self.shape
        return ops.ext().linear_fused_route(Kc, K, es)

    # -- inputs and references (CPU, cached, never modified) ----------------
    def inputs(self, outputs=0, signed=False, seed=1):
        return _inputs(self, outputs, signed, seed)

    def refs(self, inp, mode, bias=True, wq=None):
        wq = inp.wq if wq is None else wq
        b = inp.bias if bias else None
        if self.kind == "conv":
            stride, pad = self.shape[6], self.shape[7]
            return fo.conv_refs(inp.x, wq, inp.w_raw, b, stride, pad, mode)
        return fo.linear_refs(inp.x, wq, inp.w_raw, b, mode)

    # -- kernel calls -------------------------------------------------------
    def _dev(self, t):
        t = t.cuda()
        if t.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        return t

    def fused(self, inp, mode, factor, seed, telem=False, bias=True, wq=None,
              mode_int=None):
        x, wr = self._dev(inp.x), self._dev(inp.w_raw)
        wq = self._dev(inp.wq if wq is None else wq)
        b = inp.bias.cuda() if bias else torch.empty(
            0, device="cuda", dtype=self.dtype)
        f = torch.tensor([factor], device="cuda", dtype=torch.float32)
        mi = MODE_INT[mode] if mode_int is None else mode_int
        if self.kind == "conv":
            r = ops.ext().conv_fwd_fused(x, wq, wr, b, self.shape[6],
                                         self.shape[7], mi, f, seed, telem)
        else:
            r = ops.ext().linear_fwd_fused(x, wq, wr, b, mi, f, seed, telem)
        return r[0], r[1].double().cpu()

    def sigma_only(self, inp, mode, factor, seed, telem=False, mode_int=None):
        x, wr = self._dev(inp.x), self._dev(inp.w_raw)
        f = torch.tensor([factor], device="cuda", dtype=torch.float32)
        mi = MODE_INT[mode] if mode_int is None else mode_int
        if self.kind == "conv":
            r = ops.ext().sigma_noise_conv(x, wr, self.shape[6], self.shape[7],
                                           mi, f, seed, telem)
        else:
            r = ops.ext().sigma_noise_linear(x, wr, mi, f, seed, telem)
        return r[0], r[1].double().cpu()


@lru_cache(maxsize=None)
def _inputs(case, outputs, signed, seed):
    xs, ws = case.shapes(outputs)
    return fo.make_inputs(xs, ws, case.dtype, seed=seed, signed_x=signed)


@lru_cache(maxsize=8)
def _refs_cached(case, outputs, signed, mode, bias):
    return case.refs(case.inputs(outputs, signed), mode, bias)


CASES = [Case("conv", r, s, d) for r, ds, s in CONV_ROWS for d in ds] \
    + [Case("linear", r, s, d) for r, ds, s in LINEAR_ROWS for d in ds]
# the first row of every route: enough for checks that do not depend on the
# tile raggedness of the second
FIRST = [c for i, c in enumerate(CASES)
         if not any(p.kind == c.kind and p.route == c.route
                    and p.dtype == c.dtype for p in CASES[:i])]

all_cases = pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
first_cases = pytest.mark.parametrize("case", FIRST, ids=lambda c: c.id)
both_modes = pytest.mark.parametrize("mode", MODES)


# ---------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------


@all_cases
def test_row_takes_its_route(case):
    assert case.actual_route() == case.route


def test_every_route_and_dtype_is_covered():
    covered = {(c.kind, c.route, c.dtype) for c in CASES
               if c.actual_route() == c.route}
    want = set()
    for route in ("patch", "col_smallk", "col_gemm", "stream"):
        for d in ALL:
            if route == "col_smallk" and d == FP32:
                continue        # the small-K kernel is 16-bit only
            want.add(("conv", route, d))
    for route in ("smallk", "gemm"):
        for d in ALL:
            if route == "smallk" and d == FP32:
                continue
            want.add(("linear", route, d))
    print(sorted("%s/%s/%s" % (k, r, _name(d)) for k, r, d in covered))
    assert covered == want
    # and fp32 can indeed never reach the small-K kernel
    assert ops.ext().linear_fused_route(96, 65, 4) == "gemm"
    assert ops.ext().conv_fused_route(3, 15, 15, 65, 5, 5, 1, 0, 4) == "col_gemm"


def test_routes_agree_with_the_python_mirror():
    # _conv_fwd_raw keeps a Python copy of the patch predicate
    from noisynet_amd.ops.functional import _patch_eligible
    for c in CASES:
        if c.kind != "conv":
            continue
        N, C, H, W, K, R, stride, pad = c.shape
        x = torch.empty(1, C, H, W, dtype=c.dtype)
        w = torch.empty(K, C, R, R, dtype=c.dtype)
        assert _patch_eligible(x, w, pad) == (c.route == "patch"), c.id


# ---------------------------------------------------------------------------
# sigma_mode validation
# ---------------------------------------------------------------------------


def _case(kind, route, dtype=BF16):
    return next(c for c in CASES
                if (c.kind, c.route, c.dtype) == (kind, route, dtype))


@pytest.mark.parametrize("kind,route", [("conv", "stream"), ("conv", "col_gemm"),
                                        ("linear", "gemm")])
@pytest.mark.parametrize("bad", [0, 3, -1])
def test_sigma_mode_rejected_without_an_instantiation(kind, route, bad):
    case = _case(kind, route)
    inp = case.inputs()
    with pytest.raises(RuntimeError, match="sigma_mode"):
        case.fused(inp, None, 0.0, 1, mode_int=bad)
    with pytest.raises(RuntimeError, match="sigma_mode"):
        case.sigma_only(inp, None, 0.0, 1, mode_int=bad)


@pytest.mark.parametrize("kind,route", [("conv", "patch"), ("linear", "smallk"),
                                        ("conv", "col_smallk")])
def test_sigma_mode_zero_only_with_the_clean_output(kind, route):
    # these hosts have a noise-free variant, but only with the y accumulator
    case = _case(kind, route)
    inp = case.inputs()
    with pytest.raises(RuntimeError, match="sigma_mode"):
        case.sigma_only(inp, None, 0.0, 1, mode_int=0)
    with pytest.raises(RuntimeError, match="sigma_mode"):
        case.fused(inp, None, 0.0, 1, mode_int=3)
    out, _ = case.fused(inp, None, 0.0, 1, mode_int=0)
    refs = _refs_cached(case, 0, False, "abs", True)
    fo.assert_within(out, refs.clean,
                     fo.det_bound(refs.clean, refs.A, case.n, case.dtype),
                     case.id + " mode 0")


# ---------------------------------------------------------------------------
# a. clean part, every template variant
# ---------------------------------------------------------------------------


@all_cases
def test_clean_part_every_variant(case):
    inp = case.inputs()
    worst = 0.0
    for bias in (True, False):
        refs = case.refs(inp, "abs", bias)
        bound = fo.det_bound(refs.clean, refs.A, case.n, case.dtype)
        for mode in MODES:
            for telem in (True, False):
                out, _ = case.fused(inp, mode, 0.0, 5, telem, bias)
                assert out.dtype == case.dtype
                worst = max(worst, fo.assert_within(
                    out, refs.clean, bound, "%s %s bias=%d telem=%d" % (
                        case.id, mode, bias, telem)))
    for mode in MODES:
        out, _ = case.sigma_only(inp, mode, 0.0, 5)
        assert not out.float().abs().max().item(), "noise at factor 0"
    print("%s: worst ratio %.3g" % (case.id, worst))


# ---------------------------------------------------------------------------
# b. the noise ignores wq
# ---------------------------------------------------------------------------


@all_cases
def test_noise_ignores_wq(case):
    inp = case.inputs()
    wq_b = case.inputs(seed=2).wq
    ra = case.refs(inp, "abs")
    rb = case.refs(inp, "abs", wq=wq_b)
    out_a, _ = case.fused(inp, "abs", FACTOR, 77)
    out_b, _ = case.fused(inp, "abs", FACTOR, 77, wq=wq_b)
    a, b = fo.to_mk(out_a), fo.to_mk(out_b)
    # the noise term is the same fp32 number in both; each output is rounded
    # once (relative to the noisy value) and carries its own summation error
    bound = fo.U_OUT[case.dtype] * (a.abs() + b.abs()) \
        + fo.gamma(case.n) * (ra.A + rb.A)
    fo.assert_within(a - b, ra.clean - rb.clean, bound, case.id)
    assert float((a - ra.clean).abs().max()) > 0, "no noise at all"


# ---------------------------------------------------------------------------
# c. the noise field
# ---------------------------------------------------------------------------


@both_modes
@all_cases
def test_noise_field_fused(case, mode):
    inp = case.inputs(NOISE_OUTPUTS)
    refs = _refs_cached(case, NOISE_OUTPUTS, False, mode, True)
    out, _ = case.fused(inp, mode, FACTOR, 1234)
    assert NOISE_OUTPUTS <= out.numel() <= 1 << 20
    fo.check_noise_field(out, refs.clean, refs.sig, FACTOR,
                         what="%s %s" % (case.id, mode))


@both_modes
@all_cases
def test_noise_field_sigma_only(case, mode):
    inp = case.inputs(NOISE_OUTPUTS)
    refs = _refs_cached(case, NOISE_OUTPUTS, False, mode, True)
    out, _ = case.sigma_only(inp, mode, FACTOR, 4321)
    fo.check_noise_field(out, torch.zeros_like(refs.sig), refs.sig, FACTOR,
                         what="%s %s sigma-only" % (case.id, mode))


# ---------------------------------------------------------------------------
# d. seeds
# ---------------------------------------------------------------------------


@all_cases
def test_seeds(case):
    inp = case.inputs(NOISE_OUTPUTS)
    refs = _refs_cached(case, NOISE_OUTPUTS, False, "abs", True)
    o1, _ = case.fused(inp, "abs", FACTOR, 1001)
    o2, _ = case.fused(inp, "abs", FACTOR, 1001)
    o3, _ = case.fused(inp, "abs", FACTOR, 1002)
    assert torch.equal(o1, o2), "same seed, different output"
    s1, _ = case.sigma_only(inp, "abs", FACTOR, 1001)
    s2, _ = case.sigma_only(inp, "abs", FACTOR, 1001)
    assert torch.equal(s1, s2)
    sd = (FACTOR * refs.sig).sqrt()
    z1 = (fo.to_mk(o1) - refs.clean) / sd
    z3 = (fo.to_mk(o3) - refs.clean) / sd
    n = z1.numel()
    corr = float(((z1 - z1.mean()) * (z3 - z3.mean())).mean()
                 / (z1.std() * z3.std()))
    print("%s: correlation between seeds %.2f SE" % (case.id,
                                                     abs(corr) * math.sqrt(n)))
    assert abs(corr) <= 5.0 / math.sqrt(n)


# ---------------------------------------------------------------------------
# e. negative sigma
# ---------------------------------------------------------------------------

# Mode abs2 stages f(|w|) = |w|^2 + |w| as an MFMA operand, i.e. rounded once
# to the operand dtype (computed in fp32 for fp32). The kernel's sigma then
# differs from the fp64 one by up to this much relative to conv(|x|, f) on top
# of the summation bound; mode abs stages |w| exactly.
OPERAND_ROUNDING = {BF16: 2.0 ** -8, FP16: 2.0 ** -11, FP32: 2.0 ** -23}


@both_modes
@first_cases
def test_negative_sigma(case, mode):
    inp = case.inputs(NOISE_OUTPUTS, signed=True)
    refs = _refs_cached(case, NOISE_OUTPUTS, True, mode, True)
    eps = fo.gamma(case.n)
    if mode == "abs2":
        eps += OPERAND_ROUNDING[case.dtype]
    thr = eps * refs.sig_mag
    neg = refs.sig < -thr
    pos = refs.sig > thr
    frac_neg, frac_pos = float(neg.double().mean()), float(pos.double().mean())
    print("%s %s: sigma < 0 on %.3f, > 0 on %.3f of the outputs" % (
        case.id, mode, frac_neg, frac_pos))
    assert frac_neg > 0.2 and frac_pos > 0.2 and frac_neg + frac_pos > 0.9
    sig_only, _ = case.sigma_only(inp, mode, FACTOR, 99)
    so = fo.to_mk(sig_only)
    assert float(so[neg].abs().max()) == 0.0, "noise where sigma < 0"
    out, _ = case.fused(inp, mode, FACTOR, 99)
    o = fo.to_mk(out)
    bound = fo.det_bound(refs.clean, refs.A, case.n, case.dtype)
    err = (o - refs.clean).abs()
    ratio = float((err[neg] / bound[neg]).max())
    print("%s %s: clean part where sigma < 0: %.3g of the bound" % (
        case.id, mode, ratio))
    assert ratio <= 1.0
    stats = ("mean", "std")
    fo.check_noise_field(so, torch.zeros_like(refs.sig), refs.sig, FACTOR,
                         stats, case.id + " sigma-only, sigma > 0", pos, 0.2)
    fo.check_noise_field(o, refs.clean, refs.sig, FACTOR, stats,
                         case.id + " fused, sigma > 0", pos, 0.2)


# ---------------------------------------------------------------------------
# f. telemetry: all three slots
# ---------------------------------------------------------------------------


def _check_tele0(what, tele, refs):
    s_abs = float(refs.sig_abs.sum())
    rel0 = abs(float(tele[0]) - s_abs) / s_abs
    print("%s: tele0 rel err %.3g" % (what, rel0))
    assert rel0 <= TELE0_REL <= 0.02


def _check_tele(case, what, tele, out, refs):
    o = fo.to_mk(out)
    _check_tele0(what, tele, refs)
    # slot 1: sum |noise| (fp32, before the output is rounded) against
    # sum |out - clean|; deterministic, element by element
    s1 = float((o - refs.clean).abs().sum())
    b1 = float((fo.U_OUT[case.dtype] * o.abs()
                + fo.gamma(case.n) * refs.A).sum())
    e1 = abs(float(tele[1]) - s1)
    # slot 2: max of the clean fp32 y
    bm = float(fo.det_bound(refs.clean, refs.A, case.n, case.dtype).max())
    e2 = abs(float(tele[2]) - float(refs.clean.max()))
    print("%s: tele1 %.3g of bound, tele2 %.3g of bound" % (
        what, e1 / b1, e2 / bm))
    assert e1 <= b1
    assert e2 <= bm


@both_modes
@all_cases
def test_telemetry_slots(case, mode):
    inp = case.inputs()
    for bias in (True, False):
        refs = case.refs(inp, mode, bias)
        out, tele = case.fused(inp, mode, FACTOR, 31, True, bias)
        _check_tele(case, "%s %s bias=%d" % (case.id, mode, bias), tele, out,
                    refs)
    # sigma-only entry point: slot 0 is the one its callers read
    out, tele = case.sigma_only(inp, mode, FACTOR, 32, True)
    _check_tele0("%s %s sigma-only" % (case.id, mode), tele, refs)
    # and without telemetry nothing is returned
    _, none = case.fused(inp, mode, FACTOR, 31, False)
    assert none.numel() == 0


# ---------------------------------------------------------------------------
# g. public telemetry
# ---------------------------------------------------------------------------


@both_modes
@all_cases
def test_public_telemetry(case, mode):
    inp = case.inputs()
    refs = case.refs(inp, mode)
    x = inp.x.cuda()
    current, denom = 3.0, 7.0
    t = ops.NoiseTelemetry()
    torch.manual_seed(5)
    if case.kind == "conv":
        x = x.contiguous(memory_format=torch.channels_last)
        out = ops.fused_noisy_conv2d(
            x, inp.wq.cuda(), inp.w_raw.cuda(), inp.bias.cuda(),
            case.shape[6], case.shape[7], mode, FACTOR, current=current,
            power_denom=denom, want_telemetry=True, telemetry_out=t)
    else:
        out = ops.fused_noisy_linear(
            x, inp.wq.cuda(), inp.w_raw.cuda(), inp.bias.cuda(), mode, FACTOR,
            current=current, power_denom=denom, want_telemetry=True,
            telemetry_out=t)
    o = fo.to_mk(out)
    batch = inp.x.shape[0]
    # the formulas of the CPU branch, on the fp64 references
    power = 1.2e-6 * current * (float(refs.sig_abs.sum()) / batch) / denom
    s1 = float((o - refs.clean).abs().sum())
    mx = float(refs.clean.max())
    nsr = s1 / o.numel() / mx
    sparsity = float((inp.x > 0).sum()) / inp.x.numel()
    # the slot bounds of test_telemetry_slots, propagated
    b1 = float((fo.U_OUT[case.dtype] * o.abs()
                + fo.gamma(case.n) * refs.A).sum())
    bm = float(fo.det_bound(refs.clean, refs.A, case.n, case.dtype).max())
    assert mx > 2 * bm
    nsr_bound = (b1 / o.numel()) / (mx - bm) \
        + (s1 / o.numel()) * bm / (mx * (mx - bm))
    # each published value is one fp32 number: add its own rounding
    f32 = 2.0 ** -23
    got_p, got_n, got_s = float(t.power), float(t.nsr), float(t.input_sparsity)
    print("%s %s: power rel err %.3g, nsr err %.3g of bound" % (
        case.id, mode, abs(got_p - power) / power,
        abs(got_n - nsr) / nsr_bound))
    assert abs(got_p - power) <= (TELE0_REL + 4 * f32) * power
    assert abs(got_n - nsr) <= nsr_bound + 4 * f32 * nsr
    assert abs(got_s - sparsity) <= 2 * f32 * sparsity
