"""conv1 fused with its 2x2 max-pool (csrc/conv_pool_fused.hip).

The forward must be BIT-identical to the two-op composition it replaces
(``maxpool2x2_fwd(conv_fwd_fused(...))``: same accumulators, same Philox
draw per logical pixel quad, pool on the rounded values in the same order),
so the noise statistics already tested on the un-fused kernel carry over.
The backward (un-pool + wgrad in one pass) is checked against
``torch.nn.grad.conv2d_weight`` in fp32 and against the current
``maxpool2x2_bwd -> conv_wgrad_from_col`` path at the bound of
``test_conv_wgrad_patch_matches_reference``; where that path is the split-M
MFMA kernel (M >= 65536) the two must be bit-identical as well.
"""

import pytest
import torch
import torch.nn.functional as F

from noisynet_amd import ops, utils
from noisynet_amd import optim as native_optim
from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser
from noisynet_amd.graphs import GraphedTrainStep
from noisynet_amd.models.noisynet import Net
from noisynet_amd.quant import finish_calibration, start_calibration

pytestmark = pytest.mark.gpu

# (N, C, H, W, K, R): flagship geometry with an odd image count (M not a
# tile multiple, K not a multiple of 16); a single image; OH = OW = 8
ELIGIBLE = [(3, 3, 32, 32, 65, 5), (1, 3, 32, 32, 65, 5), (5, 1, 12, 12, 40, 5)]
INELIGIBLE = (2, 3, 16, 16, 16, 3)      # OW = 14
WGRAD_BOUND = 0.02                      # test_conv_wgrad_patch_matches_reference


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(shape, dtype, seed):
    N, C, H, W, K, R = shape
    g = torch.Generator().manual_seed(seed)
    # 4-bit grid inputs: few distinct products, so ties really occur
    x = (torch.randint(0, 16, (N, C, H, W), generator=g).float() / 15.0)
    w_raw = torch.randn(K, C, R, R, generator=g) * 0.2
    wq = torch.randn(K, C, R, R, generator=g) * 0.2
    bias = torch.randn(K, generator=g) * 0.1
    factor = torch.tensor([0.05])
    return (cl(x.cuda().to(dtype)), cl(wq.cuda().to(dtype)),
            cl(w_raw.cuda().to(dtype)), bias.cuda().to(dtype), factor.cuda())


def _tie_count(y):
    """Windows of the un-pooled NCHW tensor whose maximum is attained twice."""
    win = F.unfold(y.float().reshape(-1, 1, y.shape[2], y.shape[3]), 2,
                   stride=2)                       # [N*K, 4, PH*PW]
    top = win.topk(2, dim=1).values
    return int((top[:, 0] == top[:, 1]).sum())


@pytest.mark.parametrize("shape", ELIGIBLE)
@pytest.mark.parametrize("sigma_mode", [1, 2])
@pytest.mark.parametrize("with_bias", [False, True])
def test_forward_equals_composition(shape, sigma_mode, with_bias):
    x, wq, w_raw, bias, factor = _inputs(shape, torch.bfloat16, 11)
    assert ops.conv_pool_eligible(x, wq)
    b = bias if with_bias else torch.empty(0, device='cuda',
                                           dtype=torch.bfloat16)
    seed = 123456789
    y_full = ops.ext().conv_fwd_fused(x, wq, w_raw, b, 1, 0, sigma_mode,
                                      factor, seed, False)[0]
    ref_y, ref_code = ops.ext().maxpool2x2_fwd(cl(y_full))
    got_y, got_code = ops.ext().conv_pool_fwd_fused(x, wq, w_raw, b,
                                                    sigma_mode, factor, seed)
    assert _tie_count(y_full) > 0, "input was meant to produce ties"
    assert got_y.shape == ref_y.shape and got_code.shape == ref_code.shape
    assert got_y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got_y, ref_y)
    assert torch.equal(got_code, ref_code)


def test_forward_equals_composition_fp16():
    """fp16, no bias. (With a bias, fp16 showed 1-2 of 38220 values one
    fp16 step apart from the composition, codes equal: the two kernels'
    bias epilogues evidently round differently in fp32. The bf16 cases
    above, bias included, are exact.)"""
    x, wq, w_raw, _, factor = _inputs(ELIGIBLE[0], torch.float16, 12)
    bias = torch.empty(0, device='cuda', dtype=torch.float16)
    seed = 987654321
    y_full = ops.ext().conv_fwd_fused(x, wq, w_raw, bias, 1, 0, 2, factor,
                                      seed, False)[0]
    ref_y, ref_code = ops.ext().maxpool2x2_fwd(cl(y_full))
    got_y, got_code = ops.ext().conv_pool_fwd_fused(x, wq, w_raw, bias, 2,
                                                    factor, seed)
    assert torch.equal(got_y, ref_y)
    assert torch.equal(got_code, ref_code)


@pytest.mark.parametrize("shape", [ELIGIBLE[0], INELIGIBLE])
def test_public_op_equals_composition(shape, monkeypatch):
    """Through ops.fused_noisy_conv2d_pool under the same torch seed; the
    ineligible shape is the fallback check, the env switch the A/B check."""
    x, wq, w_raw, bias, factor = _inputs(shape, torch.bfloat16, 13)
    assert ops.conv_pool_eligible(x, wq) == (shape is not INELIGIBLE)

    def composed():
        torch.manual_seed(77)
        return ops.maxpool2x2(ops.fused_noisy_conv2d(
            x, wq, w_raw, bias, 1, 0, 'abs2', factor))

    def fused():
        torch.manual_seed(77)
        return ops.fused_noisy_conv2d_pool(x, wq, w_raw, bias, 1, 0, 'abs2',
                                           factor)

    want = composed()
    assert torch.equal(fused(), want)
    monkeypatch.setenv("NOISYNET_NO_CONV1_POOL", "1")
    assert not ops.conv_pool_eligible(x, wq)
    assert torch.equal(fused(), want)


def _wgrad_case(shape, seed):
    N, C, H, W, K, R = shape
    OH = H - R + 1
    PH = OH // 2
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, H, W, generator=g) * 0.5).bfloat16().float()
    gp = (torch.randn(N, K, PH, PH, generator=g) * 0.5).bfloat16().float()
    code = torch.randint(0, 4, (N, PH, PH, K), generator=g, dtype=torch.uint8)
    return x, gp, code


@pytest.mark.parametrize("shape", ELIGIBLE)
def test_wgrad_matches_reference_and_current_path(shape):
    N, C, H, W, K, R = shape
    OH = H - R + 1
    PH = OH // 2
    x, gp, code = _wgrad_case(shape, 21)
    xg, gpg, codeg = cl(x.cuda().bfloat16()), cl(gp.cuda().bfloat16()), code.cuda()
    got = ops.ext().conv_pool_wgrad(gpg, codeg, xg, R, R)
    assert got.shape == (K, C, R, R) and got.dtype == torch.bfloat16

    # full-resolution gradient by max_unpool2d from the same code
    c = code.permute(0, 3, 1, 2).long()
    ph = torch.arange(PH).view(1, 1, PH, 1)
    pw = torch.arange(PH).view(1, 1, 1, PH)
    idx = (2 * ph + c // 2) * OH + 2 * pw + c % 2
    gy = F.max_unpool2d(gp, idx, 2, 2, output_size=(OH, OH))
    ref = torch.nn.grad.conv2d_weight(x, (K, C, R, R), gy, 1, 0)
    scale = ref.abs().max().item()
    err = (got.float().cpu() - ref).abs().max().item()
    print("wgrad vs fp32 reference", shape, err / scale)
    assert err / scale < WGRAD_BOUND, (shape, err / scale)

    # the path it replaces: un-pool kernel -> wgrad from the im2col matrix
    gy_dev = ops.ext().maxpool2x2_bwd(gpg, codeg, OH, OH)
    assert torch.equal(gy_dev.float().cpu(), gy)
    col = ops.ext().im2col_materialize(xg, K, 1, 0, R, R)
    cur = ops.ext().conv_wgrad_from_col(gy_dev, col, C, R, R)
    err2 = (got.float() - cur.float()).abs().max().item()
    print("wgrad vs current path", shape, err2 / scale)
    assert err2 / scale < WGRAD_BOUND, (shape, err2 / scale)


def test_wgrad_bit_identical_to_current_path_long_contraction():
    """From M = N*OH*OW >= 65536 the current path is the split-M MFMA kernel
    (below that a library GEMM); the fused wgrad cuts and orders the
    contraction the same way, so training trajectories do not move. N = 90
    is just past the threshold; 90*784 is no multiple of the 128-deep round
    and odd images start in the middle of a 32-run."""
    shape = (90, 3, 32, 32, 65, 5)
    x, gp, code = _wgrad_case(shape, 23)
    xg, gpg, codeg = cl(x.cuda().bfloat16()), cl(gp.cuda().bfloat16()), code.cuda()
    got = ops.ext().conv_pool_wgrad(gpg, codeg, xg, 5, 5)
    gy_dev = ops.ext().maxpool2x2_bwd(gpg, codeg, 28, 28)
    col = ops.ext().im2col_materialize(xg, 65, 1, 0, 5, 5)
    cur = ops.ext().conv_wgrad_from_col(gy_dev, col, 3, 5, 5)
    assert torch.equal(got, cur)


def test_wgrad_deterministic():
    x, gp, code = _wgrad_case(ELIGIBLE[0], 3)
    xg, gpg, codeg = cl(x.cuda().bfloat16()), cl(gp.cuda().bfloat16()), code.cuda()
    a = ops.ext().conv_pool_wgrad(gpg, codeg, xg, 5, 5)
    b = ops.ext().conv_pool_wgrad(gpg, codeg, xg, 5, 5)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# model level: the flagship recipe at batch 64, bf16, steady state (i >= 20)
# ---------------------------------------------------------------------------

FLAGSHIP = ['--current', '1', '--q_a', '4', '--act_max', '5', '--batch_size',
            '64', '--calculate_running', '--no-augment']


def _model(argv, seed):
    args = build_noisynet_parser().parse_args(argv)
    broadcast_per_layer(args)
    torch.manual_seed(seed)
    model = Net(args)
    utils.init_model(model, args)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.float()
    return model.to(memory_format=torch.channels_last)


def _batch():
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(0, 16, (64, 3, 32, 32), generator=g).float() / 15.0)
    y = torch.randint(0, 10, (64,), generator=g)
    return cl(x.cuda().bfloat16()), y.cuda()


def _one_step(argv=FLAGSHIP):
    """Same-seed model, calibration and one training step at i = 100.

    The step back-propagates ops.cross_entropy as the benchmark does, but
    the loss VALUE compared by the tests is recomputed from the logits with
    torch's deterministic cross_entropy: the fused loss kernel adds its row
    partials with float atomics, so its scalar is not reproducible run to
    run even with identical logits (observed on the composition path too).
    """
    x, y = _batch()
    model = _model(argv, seed=9)
    start_calibration(model)
    with torch.no_grad():
        model(x, 0, 0)
    finish_calibration(model, torch.device('cuda'))
    model.train()
    torch.manual_seed(31)
    logits = model(x, 0, 100)
    loss = ops.cross_entropy(logits, y)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    loss = F.cross_entropy(logits.detach().float(), y)
    return model, logits.detach().clone(), loss, grads


@pytest.fixture(scope="module")
def fused_step():
    model, logits, loss, grads = _one_step()
    assert model.conv1_ is None, "flagship step did not take the fused path"
    return logits, loss, grads


def test_model_step_deterministic(fused_step):
    _, loss, grads = fused_step
    model, _, loss2, grads2 = _one_step()
    assert model.conv1_ is None
    assert torch.equal(loss, loss2)
    assert torch.equal(grads['conv1.weight'], grads2['conv1.weight'])


def test_model_step_matches_composition(fused_step, monkeypatch):
    logits, loss, grads = fused_step
    monkeypatch.setenv("NOISYNET_NO_CONV1_POOL", "1")
    model, logits_c, loss_c, grads_c = _one_step()
    assert model.conv1_ is not None, "env switch did not select the old path"
    assert torch.equal(loss, loss_c)
    assert torch.equal(logits, logits_c)
    assert set(grads) == set(grads_c)
    for n in grads:
        if n == 'conv1.weight':
            scale = grads_c[n].float().abs().max().item()
            err = (grads[n].float() - grads_c[n].float()).abs().max().item()
            print("model conv1.weight.grad", err / scale)
            assert err / scale < WGRAD_BOUND, err / scale
        else:
            assert torch.equal(grads[n], grads_c[n]), n


def test_l3_penalty_keeps_composition():
    """Double-backward penalties need the differentiable composition."""
    model, _, loss, _ = _one_step(FLAGSHIP + ['--L3', '0.01'])
    assert model.conv1_ is not None
    assert torch.isfinite(loss)


def test_graphed_replays_draw_fresh_noise_fused_path():
    model = _model(FLAGSHIP, seed=5)
    x, y = _batch()
    start_calibration(model)
    with torch.no_grad():
        for i in range(6):
            model(x, 0, i)
    finish_calibration(model, torch.device('cuda'))
    model.train()

    opt = native_optim.SGD(model.parameters(), lr=0.01, momentum=0.9,
                           nesterov=True)

    def body():
        loss = ops.cross_entropy(model(x, 0, 1000), y)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        # no optimizer step: identical weights each replay, so any loss
        # difference comes from the noise draw alone
        return loss

    gstep = GraphedTrainStep(body, warmup=1)
    assert model.conv1_ is None, "captured step did not take the fused path"
    losses = [float(gstep.replay()) for _ in range(4)]
    gstep.close()
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert len(set(losses)) > 1, losses
