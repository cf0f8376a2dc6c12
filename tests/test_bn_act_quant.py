"""ops.bn_act_quant off the GPU: the composition fallback, the model's routing
conditions and QuantMeasure.quant_range."""

import pytest
import torch

from noisynet_amd import ops, utils
from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser
from noisynet_amd.models.noisynet import Net
from noisynet_amd.quant import (QuantMeasure, finish_calibration,
                                start_calibration)


def test_cpu_is_the_composition():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 6, 6, generator=g) * 2
    w = 0.5 + torch.rand(5, generator=g)
    b = torch.rand(5, generator=g) - 0.3
    gout = torch.randn(3, 5, 6, 6, generator=g)

    def run(fused):
        xx = x.clone().requires_grad_(True)
        ww, bb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rm, rv = torch.zeros(5), torch.ones(5)
        torch.manual_seed(4)
        if fused:
            q, x_pad, mx = ops.bn_act_quant(xx, ww, bb, rm, rv, 0.1, 1e-5,
                                            2.0, 4, 0.0, 1.5, 0.5, c_pad=8)
            assert x_pad is None
        else:
            a = ops.bn_act(xx, ww, bb, rm, rv, True, 0.1, 1e-5, relu=True,
                           act_max=2.0)
            q = ops.fake_quant(a, 4, 0.0, 1.5, 0.5)
            mx = q.detach().max()
        q.backward(gout)
        return q.detach(), mx, xx.grad, ww.grad, bb.grad, rm, rv

    for a, b_ in zip(run(True), run(False)):
        assert torch.equal(a, b_)


def test_native_route_needs_16_bit_gpu_and_unsigned_range():
    x = torch.zeros(2, 8, 4, 4)
    assert not ops.bn_act_quant_native(x, None, 0.0)            # CPU fp32
    assert not ops.bn_act_quant_native(x.bfloat16(), None, 0.0)  # CPU bf16
    assert ops.conv_input_pad_width(torch.zeros(2, 65, 14, 14),
                                    torch.zeros(120, 65, 5, 5)) == 65


def _net(extra=()):
    argv = ["--current", "1", "--q_a", "4", "--act_max", "5", "--w_max1",
            "0.3", "--batch_size", "4", "--calculate_running"] + list(extra)
    args = build_noisynet_parser().parse_args(argv)
    broadcast_per_layer(args)
    torch.manual_seed(0)
    model = Net(args)
    utils.init_model(model, args)
    return model


@pytest.fixture
def calibrated(monkeypatch):
    """A calibrated flagship Net and a pooled-conv1-shaped input, with the
    device/dtype test of the native route answered 'yes' so the model's own
    conditions are what decides."""
    model = _net()
    x = torch.rand(4, 3, 32, 32)
    start_calibration(model)
    with torch.no_grad():
        for i in range(5):
            model(x, 0, i)
    finish_calibration(model)
    model.train()
    monkeypatch.setattr(ops, "bn_act_quant_native", lambda *a, **k: True)
    return model, torch.rand(4, 65, 14, 14)


def test_routing_eligible(calibrated):
    model, p = calibrated
    rng = model._bn_quant_range(p, 100)
    assert rng is not None
    lo, hi, stoch = rng
    assert lo == 0 and hi == float(model.quantize2.running_max)
    assert stoch == model.quantize2.stochastic
    assert model.quantize2.last_range == (0.0, float(hi))


def test_routing_falls_back(calibrated, monkeypatch):
    model, p = calibrated
    assert model._bn_quant_range(p, 19) is None           # telemetry batch
    model.eval()
    assert model._bn_quant_range(p, 100) is None           # eval
    model.train()
    for name, value in [("sync_bn", True), ("dropout_conv", 0.1),
                        ("q_a2", 0), ("current2", 0.0), ("batchnorm", False)]:
        old = getattr(model.args, name, None)
        setattr(model.args, name, value)
        assert model._bn_quant_range(p, 100) is None, name
        setattr(model.args, name, old)
    model.xbar_rows = 64                                    # crossbar mode
    assert model._bn_quant_range(p, 100) is None
    model.xbar_rows = 0
    model.quantize2.calculate_running = True                # calibrating
    assert model._bn_quant_range(p, 100) is None
    model.quantize2.calculate_running = False
    assert model._bn_quant_range(p, 100) is not None
    monkeypatch.setenv("NOISYNET_NO_BN_QUANT_FUSE", "1")    # the switch
    assert model._bn_quant_range(p, 100) is None
    monkeypatch.delenv("NOISYNET_NO_BN_QUANT_FUSE")
    assert model._bn_quant_range(p, 100) is not None


def test_routing_fp32_and_cpu_take_the_composition():
    """Without the monkeypatch a CPU (fp32) model never takes the route, and
    the switch changes nothing about its output."""
    model = _net()
    x = torch.rand(4, 3, 32, 32)
    start_calibration(model)
    with torch.no_grad():
        for i in range(5):
            model(x, 0, i)
    finish_calibration(model)
    model.train()
    assert model._bn_quant_range(torch.rand(4, 65, 14, 14), 100) is None
    called = []
    orig = ops.bn_act_quant
    ops.bn_act_quant = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        torch.manual_seed(1)
        model(x, 0, 100)
    finally:
        ops.bn_act_quant = orig
    assert not called


def test_quant_range_is_forwards_decision():
    q = QuantMeasure(4, stochastic=0.5, pctl=99.0)
    x = torch.rand(64) * 3
    # no fixed range yet: data-dependent, so no answer without the data and no
    # side effect
    assert q.quant_range() is None
    assert q.last_range is None and q._range_cache is None
    q.calculate_running = True
    assert q.quant_range() is None and q.running_list == []
    q(x)
    assert len(q.running_list) == 1
    q.calculate_running = False
    q.running_max = torch.tensor(2.5)
    q._range_cache = None
    q.train()
    assert q.quant_range() == (0.0, 2.5, 0.5)
    assert q.last_range == (0.0, 2.5) and q._range_cache == (0.0, 2.5)
    q.eval()
    assert q.quant_range() == (0.0, 2.5, 0)
    # forward quantises with exactly that
    q.train()
    torch.manual_seed(3)
    a = q(x)
    torch.manual_seed(3)
    b = ops.fake_quant(x, 4, 0.0, 2.5, 0.5)
    assert torch.equal(a, b)
