"""Two ranks, either on two GPUs over RCCL (backend "nccl", one device per rank: what an 8-GPU node runs) when the box
has at least two devices, or on ONE GPU over gloo (CUDA tensors moved through the host; RCCL refuses two ranks on one
device): SyncBatchNorm semantics of FusedBatchNorm2d, the DDP training step of the manager with the HIP loss, and the
shared-negative-bank all-gather.  gloo's host-staged copies synchronise the issuing stream, so only the nccl variant
can expose a missing stream dependency around a collective; every collective of the package is issued on the CURRENT
stream of the calling code (the branch's stream inside HighResolutionModule), never on a hidden one."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _backend():
    """("nccl", one device per rank) when the box has >= 2 GPUs, else ("gloo", every rank on cuda:0).  Counting devices
    does not initialise the GPU, so this is safe in the pytest parent before mp.spawn."""
    return "nccl" if torch.cuda.device_count() >= 2 else "gloo"


def _device_of(rank, backend):
    return rank if backend == "nccl" else 0


def _bn_worker(rank, world, port, out_dir, backend):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import mscs_amd  # noqa: F401
    from mscs_amd.models.fused_bn import FusedBatchNorm2d
    dev = torch.device("cuda", _device_of(rank, backend))
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    g = torch.Generator().manual_seed(5)
    shape = (4, 24, 12, 20)
    x = torch.randn(shape, generator=g) * 1.5 + 0.3
    r = torch.randn(shape, generator=g)
    gy = torch.randn(shape, generator=g)
    w = torch.rand(24, generator=g) + 0.5
    b = torch.rand(24, generator=g) - 0.5
    half = slice(2 * rank, 2 * rank + 2)
    bn = FusedBatchNorm2d(24).to(dev)
    bn.sync = True
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    xi = x[half].to(dev).requires_grad_(True)
    ri = r[half].to(dev).requires_grad_(True)
    y = bn(xi, residual=ri, relu=True)
    y.backward(gy[half].to(dev))
    out = {"y": y.detach().cpu(), "dx": xi.grad.cpu(), "dr": ri.grad.cpu(), "dw": bn.weight.grad.cpu(),
           "db": bn.bias.grad.cpu(), "rm": bn.running_mean.cpu(), "rv": bn.running_var.cpu()}
    # the same layer twice more as the two members of ONE stacked exchange (models/fused_bn.bn_act_group), the second
    # member on a side stream: must give the single-layer results
    from mscs_amd.models import fused_bn
    side = torch.cuda.Stream(device=dev)
    bns = []
    for _ in range(2):
        b2 = FusedBatchNorm2d(24).to(dev)
        b2.sync = True
        with torch.no_grad():
            b2.weight.copy_(w); b2.bias.copy_(b)
        bns.append(b2)
    xs = [x[half].to(dev).requires_grad_(True) for _ in range(2)]
    rs = [r[half].to(dev).requires_grad_(True) for _ in range(2)]
    before = fused_bn.COLLECTIVES["count"]
    torch.cuda.synchronize()
    ys = fused_bn.bn_act_group(bns, xs, residuals=rs, relu=True, streams=[None, side])
    torch.cuda.current_stream().wait_stream(side)
    ((ys[0] * gy[half].to(dev)).sum() + (ys[1] * gy[half].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    out["group_collectives"] = fused_bn.COLLECTIVES["count"] - before
    for k in range(2):
        out[f"g{k}"] = {"y": ys[k].detach().cpu(), "dx": xs[k].grad.cpu(), "dr": rs[k].grad.cpu(),
                        "dw": bns[k].weight.grad.cpu(), "rm": bns[k].running_mean.cpu()}
    torch.save(out, os.path.join(out_dir, f"bn{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_fused_bn_sync_two_ranks_one_gpu(tmp_path):
    port = _free_port()
    mp.spawn(_bn_worker, args=(2, port, str(tmp_path), _backend()), nprocs=2, join=True)
    g = torch.Generator().manual_seed(5)
    shape = (4, 24, 12, 20)
    x = (torch.randn(shape, generator=g) * 1.5 + 0.3).double().requires_grad_(True)
    r = torch.randn(shape, generator=g).double().requires_grad_(True)
    gy = torch.randn(shape, generator=g).double()
    w = torch.rand(24, generator=g) + 0.5
    b = torch.rand(24, generator=g) - 0.5
    ref = torch.nn.BatchNorm2d(24).double()
    with torch.no_grad():
        ref.weight.copy_(w); ref.bias.copy_(b)
    y = torch.relu(ref(x) + r)
    y.backward(gy)
    outs = [torch.load(os.path.join(str(tmp_path), f"bn{q}.pt")) for q in range(2)]
    for q in range(2):
        half = slice(2 * q, 2 * q + 2)
        for key, want in (("y", y.detach()[half]), ("dx", x.grad[half]), ("dr", r.grad[half])):
            assert (outs[q][key].double() - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item()), key
        assert torch.allclose(outs[q]["rm"].double(), ref.running_mean, atol=1e-5)
        assert torch.allclose(outs[q]["rv"].double(), ref.running_var, atol=1e-5)
        assert outs[q]["group_collectives"] == 2            # one stacked exchange forward, one backward
        for k in range(2):                   # the grouped (stacked-exchange) form: identical to the single layer
            for key in ("y", "dx", "dr", "dw", "rm"):
                assert torch.equal(outs[q][f"g{k}"][key], outs[q][key]), (k, key)
    # weight / bias grads are per-rank partial sums (DDP averages them): they add up to the full-batch grads
    assert torch.allclose((outs[0]["dw"] + outs[1]["dw"]).double(), ref.weight.grad, atol=2e-4)
    assert torch.allclose((outs[0]["db"] + outs[1]["db"]).double(), ref.bias.grad, atol=2e-4)


def _train_worker(rank, world, port, out_dir, global_negatives, backbone="hrnet18", scales=2, backend="gloo", no_streamk_rank=None):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import mscs_amd  # noqa: F401
    from mscs_amd.managers import HRNetManager
    from mscs_amd.utils import set_verbosity
    set_verbosity(40)
    if rank == no_streamk_rank:
        from mscs_amd import _lib
        _lib.lib().dcl_infonce_set_streamk(0)          # this rank's loss backward launches no stream-K kernel
    cfg = {"name": "t", "mode": "training", "manager": "HRNet", "cuda": True, "parallel": True,
           "gpu_device": [_device_of(q, backend) for q in range(world)], "seed": 3, "log_every_n_steps": 1000,
           "dist_backend": backend,
           "graph": {"model": "HRNet", "backbone": backbone, "sync_bn": True, "pretrained": False,
                     "align_corners": True,
                     "ms_projector": {"mlp": [[1, -1, 1]], "scales": scales, "d": 64, "use_bn": True}},
           "data": {"dataset": "CITYSCAPES", "experiment": 1, "batch_size": 4, "synthetic": True,
                    "synthetic_length": 8, "synthetic_mode": "blocky",
                    "transform_values": {"crop_shape": [64, 128]}},
           "loss": {"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1, "DenseContrastiveLossV2_ms": 0.1},
                    "temperature": 0.1, "scales": scales, "weights": [1.0, 0.5, 0.3][:scales],
                    "cross_scale_contrast": True,
                    "min_views_per_class": 2, "max_features_total": 600, "global_negatives": global_negatives},
           "train": {"learning_rate": 0.01, "lr_fct": "polynomial", "optim": "SGD", "lr_batchwise": True,
                     "epochs": 1}}
    mgr = HRNetManager(cfg, autostart=False)
    mgr.world_size = mgr.n_gpus = world
    mgr._worker_setup(_device_of(rank, backend), rank)
    mgr.train_one_epoch()
    flat = torch.cat([p.detach().flatten() for p in mgr.model.parameters()]).cpu()
    from mscs_amd.models.ops import DirectConv2d
    direct = sum(isinstance(m, DirectConv2d) for m in mgr.model.modules())
    from mscs_amd.models import fused_bn
    torch.save({"params": flat, "metrics": mgr.metrics, "direct_convs": direct, "syncbn_collectives": fused_bn.COLLECTIVES["count"],
                "syncbn_host_waits": fused_bn.COLLECTIVES["host_waits"], "backend": backend, "steps": mgr.global_step,
                "segs": [len(t.segs) for t in mgr.loss.loss_classes["DenseContrastiveLossV2_ms"].last_state.terms]},
               os.path.join(out_dir, f"train{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("global_negatives", [False, True])
def test_ddp_training_step_two_ranks_one_gpu(tmp_path, global_negatives):
    port = _free_port()
    mp.spawn(_train_worker, args=(2, port, str(tmp_path), global_negatives, "hrnet18", 2, _backend()), nprocs=2,
             join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), f"train{q}.pt")) for q in range(2)]
    assert torch.equal(a["params"], b["params"]), "parameters diverged across ranks"
    assert np.isfinite(a["metrics"]["loss"]) and np.isfinite(b["metrics"]["loss"])
    assert a["segs"] == ([2, 2, 2] if global_negatives else [1, 1, 1])


@pytest.mark.timeout(600)
def test_ddp_step_when_one_rank_runs_the_loss_backward_without_streamk(tmp_path):
    """the all-rank exchange of the stream-K error word must be issued by EVERY rank in every backward pass, also by a
    rank whose backward launched no stream-K kernel (switched off on it) -- a collective that only some ranks issue pairs up with
    the peers' next gradient bucket and hangs or corrupts the gradients.  Rank 1 runs column-split, rank 0 stream-K: the epoch
    finishes and the parameters agree bit for bit across the ranks."""
    port = _free_port()
    mp.spawn(_train_worker, args=(2, port, str(tmp_path), False, "hrnet18", 2, _backend(), 1), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), f"train{q}.pt")) for q in range(2)]
    assert torch.equal(a["params"], b["params"]), "parameters diverged across ranks"
    assert np.isfinite(a["metrics"]["loss"]) and np.isfinite(b["metrics"]["loss"])


@pytest.mark.timeout(900)
def test_ddp_hrnet48_direct_kernels_and_branch_streams_two_ranks_one_gpu(tmp_path):
    """The W48 backbone under DDP + fused SyncBatchNorm with two ranks: unlike hrnet18 its channel counts (48 / 96 /
    192 / 384, head 720) take the direct f16x3 forward, data-gradient AND weight-gradient kernels, on one HIP stream
    per branch, with the blocking per-norm all-reduce between the statistics and the apply kernels -- the schedule
    that runs on an 8-GPU node (there over RCCL; gloo here because both ranks share the one GPU of this box).
    Shared negative bank on: the overlapped per-scale bank gathers run too."""
    port = _free_port()
    mp.spawn(_train_worker, args=(2, port, str(tmp_path), True, "hrnet48", 3, _backend()), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), f"train{q}.pt")) for q in range(2)]
    assert a["direct_convs"] > 250                                   # every 3x3 convolution of W48 is a DirectConv2d
    assert torch.equal(a["params"], b["params"]), "parameters diverged across ranks"
    assert np.isfinite(a["metrics"]["loss"]) and np.isfinite(b["metrics"]["loss"])
    assert a["segs"] == [2] * 5                                      # 3 intra + 2 cross terms, 2 segments each
    # SyncBatchNorm exchanges per step: 310 norms x 2 directions = 620 one by one; the branch chains' 208 norms share one
    # exchange per block depth (64 instead of 208 per direction)
    per_step = a["syncbn_collectives"] / max(1, a["steps"])
    assert per_step <= 340, per_step
    # every exchange is issued asynchronously and awaited on the STREAM right before its consumer (fused_bn._Exchange): on RCCL
    # (DCL_TEST_BACKEND=nccl, a node with two GPUs) the host never waits; gloo -- the stand-in on one-GPU boxes -- completes
    # every collective on the host
    assert a["syncbn_host_waits"] == (0 if a["backend"] == "nccl" else a["syncbn_collectives"])


def _rank_setup(rank, world, port, backend):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import mscs_amd  # noqa: F401
    dev = torch.device("cuda", _device_of(rank, backend))
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    return dev


_PRE_SHAPE, _PRE_CO = (4, 32, 16, 32), 48


def _pre_inputs():
    g = torch.Generator().manual_seed(11)
    n, c, h, w = _PRE_SHAPE
    x = torch.randn(_PRE_SHAPE, generator=g) * 1.3 + 2.0 * torch.randn(1, c, 1, 1, generator=g)
    x[:2] += 0.5                                        # the two halves differ: per-rank statistics are not the global ones
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::5] *= -1.0
    beta = torch.randn(c, generator=g) * 0.5
    beta[3::7] += 3.0                                   # relu(sh) >> 0 on these channels: the zero border must stay zero
    wt = torch.randn(_PRE_CO, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5
    gy = torch.randn(n, _PRE_CO, h, w, generator=g)
    return x, gamma, beta, wt, gy


def _pre_worker(rank, world, port, out_dir, backend):
    """deferred FusedBatchNorm2d(sync=True) -> PRE DirectConv2d 3x3 on this rank's half: the launch sequence
    dcl_bn_stats_minmax_part -> all-reduce -> dcl_bn_finalize_pre with this rank's extrema"""
    dev = _rank_setup(rank, world, port, backend)
    from mscs_amd.models.amax import pre_of
    from mscs_amd.models.fused_bn import FusedBatchNorm2d
    from mscs_amd.models.ops import DirectConv2d
    x, gamma, beta, wt, gy = _pre_inputs()
    c = x.shape[1]
    half = slice(2 * rank, 2 * rank + 2)
    bn = FusedBatchNorm2d(c).to(dev)
    bn.sync = True
    conv = DirectConv2d(c, _PRE_CO, 3, padding=1, bias=False).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); conv.weight.copy_(wt)
    xi = x[half].to(dev).requires_grad_(True)
    assert conv.fuses_input_norm(xi)
    y = bn(xi, relu=True, defer=True)
    pre = pre_of(y)
    assert pre is not None and y.data_ptr() == xi.data_ptr()
    out = conv(y)
    out.backward(gy[half].to(dev))
    c4 = (1, c, 1, 1)
    mapped = torch.addcmul(pre.sh.view(c4).double(), xi.detach().double(), pre.sc.view(c4).double()).float().relu_()
    torch.save({"y": out.detach().cpu(), "dx": xi.grad.cpu(), "dgamma": bn.weight.grad.cpu(), "dbeta": bn.bias.grad.cpu(),
                "dw": conv.weight.grad.cpu(), "rm": bn.running_mean.cpu(), "rv": bn.running_var.cpu(),
                "amax": pre.amax.max().item(), "amax_want": mapped.max().item()}, os.path.join(out_dir, f"pre{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _close(got, want, bar=2e-5):
    return (got.double() - want).abs().max().item() <= bar * max(want.abs().max().item(), 1e-12)


@pytest.mark.timeout(300)
def test_deferred_sync_bn_into_pre_convolution_two_ranks(tmp_path):
    """Two ranks, each with half the batch, against the full-batch float64 composition conv3x3(relu(bn(x))): output and input
    gradient of each half, running statistics at 2e-5 of max; the ranks' gradients of gamma, beta and the convolution weight add up
    to the full-batch ones; the absmax of each rank's mapped half exact."""
    port = _free_port()
    mp.spawn(_pre_worker, args=(2, port, str(tmp_path), _backend()), nprocs=2, join=True)
    x, gamma, beta, wt, gy = _pre_inputs()
    c = x.shape[1]
    bn = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    w64 = wt.double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(torch.relu(bn(xr)), w64, None, 1, 1)
    y.backward(gy.double())
    outs = [torch.load(os.path.join(str(tmp_path), f"pre{q}.pt")) for q in range(2)]
    for q in range(2):
        half = slice(2 * q, 2 * q + 2)
        assert _close(outs[q]["y"], y.detach()[half]), ("y", q)
        assert _close(outs[q]["dx"], xr.grad[half]), ("dx", q)
        assert _close(outs[q]["rm"], bn.running_mean) and _close(outs[q]["rv"], bn.running_var), ("running statistics", q)
        assert outs[q]["amax"] == outs[q]["amax_want"], q
    for key, want in (("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad), ("dw", w64.grad)):
        assert _close(outs[0][key] + outs[1][key], want), key


_HEAD_SHAPE, _HEAD_K = (4, 37, 6, 12), 19


def _head_inputs(r):
    g = torch.Generator().manual_seed(13)
    n, c, h, w = _HEAD_SHAPE
    std = torch.rand(1, c, 1, 1, generator=g) + 0.5
    z = torch.randn(_HEAD_SHAPE, generator=g) * std + r * std * torch.where(torch.rand(1, c, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    z[:2] += 0.3 * std                                  # the halves differ
    gl = torch.randn(n, _HEAD_K, h, w, generator=g) * 1e-3
    wt = torch.randn(_HEAD_K, c, 1, 1, generator=g) * (1.0 / c) ** 0.5
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::7] *= -1.0
    beta = torch.randn(c, generator=g) * 0.3
    return z, gl, wt, gamma, beta


_HEAD_RATIOS = (0.3, 30.0)


def _head_worker(rank, world, port, out_dir, backend):
    """HRNet._head_tail with bn.sync = True on this rank's half: one warm-up call (the guard sees the layer's running statistics),
    then forward + backward; at r = 0.3 the fold (all-reduced statistics and channel sums, per-rank dgamma / dbeta / dW), at r = 30
    the unfolded SyncBatchNorm -- the same decision on both ranks"""
    dev = _rank_setup(rank, world, port, backend)
    import importlib
    import types
    from mscs_amd.models.fused_bn import FusedBatchNorm2d
    from mscs_amd.models.ops import DirectConv2d
    H = importlib.import_module("mscs_amd.models.HRNet")
    half = slice(2 * rank, 2 * rank + 2)
    res = {}
    for r in _HEAD_RATIOS:
        z, gl, wt, gamma, beta = _head_inputs(r)
        c = z.shape[1]
        bn = FusedBatchNorm2d(c).to(dev)
        bn.sync = True
        cls = DirectConv2d(c, _HEAD_K, 1, bias=False).to(dev)
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta); cls.weight.copy_(wt)
            bn.running_mean.copy_(z.double().mean((0, 2, 3)).float()); bn.running_var.copy_(z.double().var((0, 2, 3)).float())
        head = types.SimpleNamespace(cls_head=torch.nn.Sequential(torch.nn.Identity(), bn, cls).train())
        zi = z[half].to(dev)
        with torch.no_grad():
            H.HRNet._head_tail(head, zi)                # warm-up
        rm0, rv0 = bn.running_mean.cpu(), bn.running_var.cpu()
        zf = zi.clone().requires_grad_(True)
        out = H.HRNet._head_tail(head, zf)
        node = type(out.grad_fn).__name__
        out.backward(gl[half].to(dev))
        res[r] = {"node": node, "y": out.detach().cpu(), "dz": zf.grad.cpu(), "dgamma": bn.weight.grad.cpu(),
                  "dbeta": bn.bias.grad.cpu(), "dw": cls.weight.grad.cpu(), "rm0": rm0, "rv0": rv0,
                  "rm": bn.running_mean.cpu(), "rv": bn.running_var.cpu()}
    torch.save(res, os.path.join(out_dir, f"head{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_folded_head_sync_bn_two_ranks(tmp_path):
    """Two ranks against the full-batch float64 conv1x1(bn(z)): logits and dz of each half and the running statistics at 2e-5 of
    max; dgamma, dbeta and dW of the two ranks add up to the full-batch ones.  Both ranks take the same path: the fold at
    r = |mean| / std = 0.3, the unfolded norm at r = 30 (ops_head.FOLD_MAX_MEAN_RATIO)."""
    port = _free_port()
    mp.spawn(_head_worker, args=(2, port, str(tmp_path), _backend()), nprocs=2, join=True)
    outs = [torch.load(os.path.join(str(tmp_path), f"head{q}.pt")) for q in range(2)]
    for r in _HEAD_RATIOS:
        nodes = [outs[q][r]["node"] for q in range(2)]
        assert nodes[0] == nodes[1], (r, nodes)
        assert (nodes[0] == "_HeadNormClassifierBackward") == (r < 1), (r, nodes)
        z, gl, wt, gamma, beta = _head_inputs(r)
        c = z.shape[1]
        assert torch.equal(outs[0][r]["rm0"], outs[1][r]["rm0"]) and torch.equal(outs[0][r]["rv0"], outs[1][r]["rv0"])
        bn = torch.nn.BatchNorm2d(c).double()
        conv = torch.nn.Conv2d(c, _HEAD_K, 1, bias=False).double()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta); conv.weight.copy_(wt)
            bn.running_mean.copy_(outs[0][r]["rm0"]); bn.running_var.copy_(outs[0][r]["rv0"])
        zr = z.double().requires_grad_(True)
        y = conv(bn(zr))
        y.backward(gl.double())
        for q in range(2):
            half = slice(2 * q, 2 * q + 2)
            o = outs[q][r]
            assert _close(o["y"], y.detach()[half]), ("logits", r, q)
            assert _close(o["dz"], zr.grad[half]), ("dz", r, q)
            assert _close(o["rm"], bn.running_mean) and _close(o["rv"], bn.running_var), ("running statistics", r, q)
        for key, want in (("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad), ("dw", conv.weight.grad)):
            assert _close(outs[0][r][key] + outs[1][r][key], want), (key, r)
