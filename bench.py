#!/usr/bin/env python3
"""Flagship benchmark: NoisyNet 4-layer CIFAR-10 ConvNet, 4-bit quantized
activations (q_a=4, the README flagship config leaves weights unquantized),
analog noise I_max=1nA, act_max=5, bf16, synthetic 4-bit-CIFAR-shaped data
(BASELINE.json metric: images/sec whole node + top-1).

Single GPU:       python bench.py --steps 100 --warmup 20
Multi-GPU (driver): python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...
Accuracy:         python bench.py --full --top1 30   (trains the flagship on
    the learnable synthetic CIFAR and reports held-out top-1 in the JSON line)
Outputs:          python bench.py --dump-outputs DIR   (writes what the last
    timed step computed as DIR/<name>.npy, to compare two builds)

A plain run only sets up, warms up, times --steps steps and prints the
result line. Everything that takes runs of its own (today: the --top1
accuracy run) sits behind --full.

Weak scaling: per-GPU batch is fixed (--batch), global batch = N * batch.
Each timed step is a FULL training step on a FRESH batch sliced from a
GPU-resident dataset, with the reference's GPU crop/flip augmentation
(noisynet.py:1261-1269) inside the timed region: forward (fused
quant+conv+sigma+noise kernels), fused softmax-xent, backward (dgrad/
wgrad), bucketed RCCL all-reduce overlapped with backward, fused AdamW
update with the weight clamp folded in (the recipe's default optimizer).
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from noisynet_amd import data as data_mod  # noqa: E402
from noisynet_amd import distributed as dist_mod  # noqa: E402
from noisynet_amd import ops  # noqa: E402
from noisynet_amd import optim as native_optim  # noqa: E402
from noisynet_amd import utils  # noqa: E402
from noisynet_amd.config import broadcast_per_layer, build_noisynet_parser  # noqa: E402
from noisynet_amd.models.noisynet import Net  # noqa: E402
from noisynet_amd.quant import finish_calibration, start_calibration  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--model", type=str, default="noisynet",
                   choices=["noisynet", "resnet18", "mobilenet_v2",
                            "efficientnet_b0"],
                   help="BASELINE.json configs 2-5; default = flagship")
    p.add_argument("--batch", type=int, default=0,
                   help="per-GPU batch size (weak scaling); 0 = per-model default")
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["bf16", "fp32"])
    p.add_argument("--no-noise", action="store_true",
                   help="disable analog/weight noise (noise-free baseline)")
    p.add_argument("--no-augment", action="store_true",
                   help="skip the in-loop GPU crop/flip (flagship only)")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure (today: the --top1 accuracy run)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step computed (loss, gradients, updated parameters "
                        "and buffers) as DIR/<name>.npy")
    p.add_argument("--top1", type=int, default=0, metavar="EPOCHS",
                   help="with --full: after the throughput run, train the "
                        "flagship on the learnable synthetic CIFAR for "
                        "EPOCHS epochs and "
                        "report held-out top-1 (the accuracy half of the "
                        "BASELINE metric)")
    p.add_argument("--graph", action="store_true", default=None,
                   help="capture the training step in a hipGraph (default: "
                        "auto per model)")
    p.add_argument("--no-graph", dest="graph", action="store_false")
    p.add_argument("--seed", type=int, default=42)
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if args.top1 > 0 and not args.full:
        p.error("--top1 is part of the full run: add --full")
    if args.batch == 0:
        # throughput-optimal per-GPU batch on 288 GB HBM3E (weak scaling
        # keeps this fixed as N grows). Sweep-measured: flagship 8192 ->
        # 16384 -> 32768 = 670 -> 691 -> 700k img/s; secondary models were
        # batch-starved at 256 (ResNet-18 63k -> 121k @1024, EffNet-B0
        # 10.5k -> 15.0k, MNv2 9.2k -> 11.3k; 2048 adds a little more:
        # 148k / 16.0k / 11.6k)
        args.batch = 32768 if args.model == "noisynet" else 1024
    return args


def flagship_args(bench):
    """BASELINE.json config 2: NoisyNet CIFAR-10 4-bit, I_max=1nA, act_max=5."""
    argv = ["--q_a", "4", "--act_max", "5", "--w_max1", "0.3",
            "--LR", "0.005", "--L2_1", "0.0005", "--L2_2", "0.0002",
            "--batch_size", str(bench.batch), "--calculate_running"]
    if bench.no_augment:
        argv += ["--no-augment"]
    if not bench.no_noise:
        argv = ["--current", "1"] + argv
    args = build_noisynet_parser().parse_args(argv)
    broadcast_per_layer(args)
    return args


def build_secondary(bench, device, dtype):
    """BASELINE.json configs 3-5: ResNet-18 CIFAR-shaped 4-bit + weight
    noise; MobileNetV2 / EfficientNet-B0 ImageNet-shaped quant-aware."""
    from noisynet_amd.config import build_main_parser

    if bench.model == "resnet18":
        argv = ["-a", "resnet18", "--q_a", "4", "--q_w", "4",
                "--calculate_running"]
        if not bench.no_noise:
            argv += ["--n_w", "0.1"]
        image_size, num_classes = 32, 10   # CIFAR-10-shaped (config 3)
    else:
        argv = ["-a", bench.model, "--q_a", "4", "--calculate_running"]
        image_size, num_classes = 224, 1000
    args = build_main_parser().parse_args(argv)

    if bench.model == "resnet18":
        from noisynet_amd.models.resnet import ResNet18
        model = ResNet18(args)
        # CIFAR-10 head
        from noisynet_amd.hardware_model import NoisyLinear
        model.fc = NoisyLinear(512, num_classes, bias=True, num_bits=0,
                               num_bits_weight=args.q_w, noise=args.n_w,
                               test_noise=args.n_w_test,
                               stochastic=args.stochastic)
    elif bench.model == "mobilenet_v2":
        from noisynet_amd.models.mobilenet import mobilenet_v2
        model = mobilenet_v2(args)
    else:
        from noisynet_amd.timm.models import create_model
        model = create_model("efficientnet_b0", num_classes=num_classes)
        model.args = args
    model = model.to(device)
    if dtype is torch.bfloat16:
        model = model.bfloat16()
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.float()
    if device.type == "cuda":
        model = model.to(memory_format=torch.channels_last)
    return model, args, image_size, num_classes


def run_top1(bench, device, dtype, rank, distributed):
    """Train the flagship to convergence on the learnable synthetic CIFAR
    and return held-out top-1 (the accuracy half of the BASELINE metric,
    reference README.md:6-13 semantics on synthetic data)."""
    args = flagship_args(bench)
    args.batch_size = 64  # the reference recipe's batch (noisynet.py default)
    args.augment = True
    torch.manual_seed(bench.seed)
    model = Net(args)
    utils.init_model(model, args)
    model = model.to(device)
    if device.type == "cuda":
        model = model.to(memory_format=torch.channels_last)

    tr, trl, te, tel = data_mod.synthesize_cifar4bit(50000, 10000)
    X = torch.from_numpy(tr).to(device)
    X = torch.nn.functional.pad(X, (4, 4, 4, 4))
    y = torch.from_numpy(trl).to(device)
    Xt = torch.from_numpy(te).to(device)
    yt = torch.from_numpy(tel).to(device)
    if device.type == "cuda":
        X = X.contiguous(memory_format=torch.channels_last)
        Xt = Xt.contiguous(memory_format=torch.channels_last)

    param_groups = [
        {"params": model.conv1.parameters(), "weight_decay": args.L2_1,
         "lr": args.LR, "clamp": (-args.w_max1, args.w_max1)},
        {"params": model.conv2.parameters(), "weight_decay": args.L2_2,
         "lr": args.LR},
        {"params": model.linear1.parameters(), "weight_decay": args.L2_3,
         "lr": args.LR},
        {"params": model.linear2.parameters(), "weight_decay": args.L2_4,
         "lr": args.LR},
        {"params": [p for m in (model.bn1, model.bn2, model.bn3, model.bn4)
                    for p in m.parameters()], "weight_decay": 0.0,
         "lr": args.LR},
    ]
    # the recipe's real optimizer: AdamW (reference noisynet.py:249 default)
    optimizer = native_optim.AdamW(param_groups, lr=args.LR)
    bs = args.batch_size
    n = X.shape[0]
    start_calibration(model)
    curve = []
    for epoch in range(bench.top1):
        # step LR decay, as in tools/accuracy_curve.py (constant LR left
        # late epochs unstable)
        if epoch in (int(bench.top1 * 0.5), int(bench.top1 * 0.75),
                     int(bench.top1 * 0.9)):
            for group in optimizer.param_groups:
                group['lr'] *= 0.2
        model.train()
        perm = torch.randperm(n, device=device)
        for i in range(n // bs):
            idx = perm[i * bs:(i + 1) * bs]
            xb = data_mod.gpu_augment(X[idx])
            if epoch == 0 and i == 5:
                finish_calibration(model, device)
            out = model(xb, epoch, i)
            loss = ops.cross_entropy(out, y[idx])
            optimizer.zero_grad(set_to_none=False)
            loss.backward()
            optimizer.step()
        model.eval()
        correct = 0
        with torch.no_grad():
            for i in range(0, Xt.shape[0], 1000):
                out = model(Xt[i:i + 1000], epoch, 100)
                correct += int((out.argmax(1) == yt[i:i + 1000]).sum())
        acc = 100.0 * correct / Xt.shape[0]
        curve.append(round(acc, 2))
        if rank == 0:
            print("# top1 epoch %d: %.2f%%" % (epoch, acc), file=sys.stderr)
    return curve


DUMP_BUDGET_BYTES = 48 << 20  # whole dump stays well under 64 MB


def dump_outputs(out_dir, loss, model):
    """Write what the last timed step left behind -- the loss it returned,
    the gradients it computed, the parameters and buffers it updated -- as
    float32 (float64 for integer buffers) ``<name>.npy`` files. Arrays that
    would overflow the byte budget are cut to a fixed seeded sample."""
    import numpy as np

    arrays = {"loss": loss.detach()}
    for name, p in model.named_parameters():
        arrays["param." + name] = p.detach()
        if p.grad is not None:
            arrays["grad." + name] = p.grad.detach()
    for name, b in model.named_buffers():
        arrays["buffer." + name] = b.detach()

    total = sum(t.numel() * (4 if t.is_floating_point() else 8)
                for t in arrays.values())
    keep = min(1.0, DUMP_BUDGET_BYTES / max(total, 1))
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.RandomState(1234)
    for name, t in arrays.items():
        a = t.to("cpu", torch.float32 if t.is_floating_point()
                 else torch.float64).contiguous().numpy().reshape(-1)
        if keep < 1.0 and a.size > 1024:
            idx = np.sort(rng.choice(a.size, int(a.size * keep),
                                     replace=False))
            a = a[idx]
        else:
            a = a.reshape(tuple(t.shape))
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    bench = parse_args()
    torch.manual_seed(bench.seed)

    world_size = dist_mod.env_world_size()
    rank = dist_mod.env_rank()
    distributed = dist_mod.init_distributed()
    n_gpus = world_size if distributed else 1

    if torch.cuda.is_available():
        device = torch.device("cuda", dist_mod.env_local_rank())
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    dtype = torch.bfloat16 if bench.dtype == "bf16" else torch.float32

    if bench.model == "noisynet":
        args = flagship_args(bench)
        model = Net(args)
        utils.init_model(model, args)
        model = model.to(device)
        if dtype is torch.bfloat16:
            model = model.bfloat16()
            # BN statistics stay fp32 for stability
            for m in model.modules():
                if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    m.float()
        if device.type == "cuda":
            model = model.to(memory_format=torch.channels_last)
        image_size, num_classes = 32, 10
    else:
        model, args, image_size, num_classes = build_secondary(bench, device,
                                                               dtype)

    dp = dist_mod.DataParallel(model) if distributed else None

    # GPU-resident synthetic 4-bit-grid dataset, several batches deep so
    # every timed step sees a fresh slice (reference noisynet.py:1249-1276)
    flagship = bench.model == "noisynet"
    augment = flagship and not bench.no_augment
    n_slices = 4
    g = torch.Generator().manual_seed(bench.seed + rank)
    store = image_size + 8 if augment else image_size
    data = (torch.randint(0, 16,
                          (bench.batch * n_slices, 3, store, store),
                          generator=g).to(device=device, dtype=dtype) / 15.0)
    if device.type == "cuda":
        data = data.contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, num_classes, (bench.batch * n_slices,),
                           generator=g).to(device)

    if bench.model == "noisynet":
        param_groups = [
            {"params": model.conv1.parameters(), "weight_decay": args.L2_1,
             "lr": args.LR, "clamp": (-args.w_max1, args.w_max1)},
            {"params": model.conv2.parameters(), "weight_decay": args.L2_2,
             "lr": args.LR},
            {"params": model.linear1.parameters(), "weight_decay": args.L2_3,
             "lr": args.LR},
            {"params": model.linear2.parameters(), "weight_decay": args.L2_4,
             "lr": args.LR},
            {"params": [p for m in (model.bn1, model.bn2, model.bn3, model.bn4)
                        for p in m.parameters()], "weight_decay": 0.0,
             "lr": args.LR},
        ]
        # fused AdamW: the flagship recipe's default optimizer
        # (reference noisynet.py:249)
        optimizer = native_optim.AdamW(param_groups, lr=args.LR)
    else:
        optimizer = native_optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                                     weight_decay=1e-4, nesterov=False)

    # hipGraph capture: one graph launch per step instead of ~900 host
    # launches (decisive for the host-bound secondary models). Single
    # process only -- the multi-GPU path keeps eager launches so the
    # bucketed RCCL all-reduce can overlap backward.
    use_graph = bench.graph
    if use_graph is None:
        # auto: the deep many-launch models gain (ResNet-18 35.6k -> 53.3k
        # img/s measured); the flagship's 4-layer step is already 88% GPU
        # busy and the static-buffer copies cost more than the host gap
        use_graph = bench.model != "noisynet"
    use_graph = use_graph and device.type == "cuda" and not distributed

    def eager_step(i):
        model.train()
        s = (i % n_slices) * bench.batch
        xb = data[s:s + bench.batch]
        if augment:
            xb = data_mod.gpu_augment(xb)
        yb = labels[s:s + bench.batch]
        out = model(xb, 0, i) if bench.model != "efficientnet_b0" \
            else model(xb)
        loss = ops.cross_entropy(out, yb)
        optimizer.zero_grad(set_to_none=False)
        loss.backward()
        if dp is not None:
            dp.finish()
        optimizer.step()
        return loss

    # calibration (5 batches) then freeze ranges, as the reference does
    start_calibration(model)
    with torch.no_grad():
        for i in range(5):
            xb = data[:bench.batch]
            if augment:
                xb = data_mod.gpu_augment(xb)
            model(xb, 0, i) if bench.model != "efficientnet_b0" else model(xb)
    finish_calibration(model, device)

    if use_graph:
        from noisynet_amd.graphs import GraphedTrainStep

        static_x = torch.empty(bench.batch, 3, image_size, image_size,
                               device=device, dtype=dtype).contiguous(
                                   memory_format=torch.channels_last)
        static_y = torch.empty(bench.batch, dtype=torch.int64, device=device)

        def fill(i):
            s = (i % n_slices) * bench.batch
            xb = data[s:s + bench.batch]
            if augment:
                xb = data_mod.gpu_augment(xb)
            static_x.copy_(xb)
            static_y.copy_(labels[s:s + bench.batch])

        def graph_body():
            out = model(static_x, 0, 1000) \
                if bench.model != "efficientnet_b0" else model(static_x)
            loss = ops.cross_entropy(out, static_y)
            optimizer.zero_grad(set_to_none=False)
            loss.backward()
            optimizer.step()
            return loss

        model.train()
        fill(0)
        gstep = GraphedTrainStep(graph_body)

        def step(i):
            fill(i)
            return gstep.replay()
    else:
        step = eager_step

    for i in range(bench.warmup):
        step(i + 100)  # i>=20: telemetry off in steady state

    if distributed:
        torch.distributed.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(bench.steps):
        last_loss = step(i + 1000).detach()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    if distributed:
        torch.distributed.barrier()

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64)
    if distributed:
        elapsed = elapsed.to(device if device.type == "cuda" else "cpu")
        torch.distributed.all_reduce(elapsed, op=torch.distributed.ReduceOp.MAX)
    elapsed = float(elapsed.item())

    ms_per_step = elapsed / bench.steps * 1000.0
    images_per_sec = n_gpus * bench.batch * bench.steps / elapsed

    if bench.dump_outputs and rank == 0:
        dump_outputs(bench.dump_outputs, last_loss, model)

    top1_curve = None
    if bench.full and bench.top1 > 0 and bench.model == "noisynet":
        top1_curve = run_top1(bench, device, dtype, rank, distributed)

    if rank == 0:
        out = {
            "metric": "images/sec (whole node) + top-1, NoisyNet 4-bit "
                      "CIFAR-10 I_max=1nA, 1/2/4/8 GPU",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": bench.steps,
            "warmup": bench.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": bench.dtype,
            "data": "synthetic",
            "config": {
                "model": ("noisynet-4layer-cifar" if bench.model == "noisynet"
                          else bench.model),
                "global_batch": n_gpus * bench.batch,
                "seq_len": None,
                "image_size": image_size,
                "augment": bool(augment),
                "hip_graph": bool(use_graph),
                "q_a": 4,
                "q_w": 4 if bench.model == "resnet18" else 0,
                "current_nA": (0 if (bench.no_noise or bench.model != "noisynet")
                               else 1),
                "act_max": 5 if bench.model == "noisynet" else 0,
                "optim": ("adamw" if bench.model == "noisynet" else "sgd"),
                "parallelism": "dp%d" % n_gpus,
            },
        }
        if top1_curve is not None:
            out["top1"] = top1_curve[-1]
            out["top1_curve"] = top1_curve
            out["top1_epochs"] = bench.top1
        print(json.dumps(out))

    sys.stdout.flush()
    if distributed:
        try:
            torch.distributed.destroy_process_group()
        except Exception:
            pass  # teardown must never invalidate the printed result


if __name__ == "__main__":
    main()
